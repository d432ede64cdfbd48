"""Evaluation loop -- the ``mlp/test.py`` entry point on the HIP path.

``testing(dataset, model, loss, total_iter, mode, train_start_time)`` keeps the reference's
signature, per-recipe metric routing (mlp/test.py:43-92) and returned dict (:138-145).  The
model/loss calls run on the GPU.  The counters are accumulated ON THE GPU and the loss is summed there
too (``opt.device_metrics``) instead of the reference's per-batch ``.item()`` + ``.cpu()``
of every logit (:42, :50-67): by ``lirec_eval_max_tracks`` for the max-over-tracks recipes
(``tr_maximize``), by ``lirec_eval_clip_topk`` (top-1 / 3 / 5, soft labels, confusion matrix) for the
others.  The per-pair relationship scores of ``rels_multitask`` are the one thing still summed on the
host: their logits wait in a device buffer and come back in ONE copy after the loop, so the sums keep
the host path's order bit for bit.  ``device_metrics=False`` and ``ints != 1`` keep the host
counters on logits copied back once per batch.  Differences, on purpose: no interaction-name file is
read (:29-32 only builds an unused table), and clips/s is printed next to the metrics.
``opt.record_eval`` (off by default) over a resident block store: the forward-only iteration is recorded on the second full batch
and replayed for the rest (``lirec_amd.graph.EvalStepper``) -- the same bits.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import ops
from ._lib import LirecError
from .config import opt
from .graph import EvalStepper, RecordedEvalStep
from .loader import _Cursor, make_loader
from .metrics import Precision, RelationshipsAcc
from .util import Averaging


def testing(test_dataset, model, loss, total_iter=1, mode='val', train_start_time='', verbose=True):
    # One process per GPU (lirec_amd.parallel): each rank evaluates ITS clips of the dataset (every clip on exactly one rank), the
    # counters are summed over the ranks after the loop and every rank returns -- rank 0 prints -- the whole dataset's metrics
    # (mlp/test.py:94-145 prints one set).  COLLECTIVE under torch.distributed: every rank calls testing() at the same point.
    from . import parallel
    rank, world = parallel.world_info()
    sharded = world > 1 and bool(getattr(opt, 'dp_shard_eval', True))
    sampler = parallel.ShardSampler(len(test_dataset), opt.batch_size, shuffle=False, pad=False) if sharded else None
    verbose = verbose and (rank == 0 or not sharded)
    loader = make_loader(test_dataset, opt.batch_size, sampler=sampler)
    losses = Averaging()
    model.eval()
    prec = Precision(inter2mgd=getattr(test_dataset, 'interidx2mgdidx', None), n_rels=opt.rels_dim, soft_gt=opt.soft_gt)
    n_rels = test_dataset.n_rels                      # dataset-side count, includes "None"
    prec_rels = RelationshipsAcc(n_rels=n_rels) if opt.rels_multitask else None
    conf_mat = np.zeros((test_dataset.n_classes, test_dataset.n_classes))
    total_tracks, n_clips, t0 = 0, 0, time.time()
    on_device = bool(getattr(opt, 'device_metrics', True)) and opt.tr_maximize and not opt.soft_gt and opt.ints == 1
    # the recipes without a maximum over tracks: clip-level counters by lirec_eval_clip_topk
    on_device_topk = (bool(getattr(opt, 'device_metrics', True)) and str(opt.device).startswith('cuda') and opt.ints == 1
                      and not opt.tr_maximize)
    dev_counters = dev_loss = dev_conf = dev_rels = dev_tracks = None
    n_batches = n_out = rels_at = 0
    rels_parts = []                                   # (offset, rows, labelled rows, their labels, their pair hashes) per batch
    to_dev = getattr(test_dataset, 'to_device', None) if (on_device and str(opt.device).startswith('cuda')) else None
    # opt.record_eval over a resident block store, one process, device-side counters: the iteration is recorded on the second full
    # batch and replayed for the rest (lirec_amd.graph.EvalStepper).  None: the loop below, exactly.
    stepper = rec = None
    if EvalStepper.wanted(loader, world) and (on_device or on_device_topk) and to_dev is None and str(opt.device).startswith('cuda'):
        stepper = EvalStepper(model, loader, loss=loss, say=print if verbose else (lambda *a, **k: None))
        rec = {'cursor': _Cursor(torch.device(opt.device)), 'labels': None, 'hashes': None}

    def keep_rows(t, buf):
        """rows of an int64 batch field into a dataset-sized buffer at the output cursor -- 8-byte values moved as fp32 pairs"""
        rows = t.reshape(t.shape[0], -1).view(torch.float32)
        if buf is None:
            buf = torch.empty(dev_rels.shape[0], rows.shape[1], dtype=torch.float32, device=rows.device)
        ops.rows_copy_at(rows, buf, rec['cursor'].word)
        return buf

    def kept_rows(buf, like, at, bs):
        return buf[at:at + bs].view(torch.int64).reshape((bs,) + tuple(like.shape[1:]))

    def recorded_tail(out, batch):
        """the device part of one iteration below in LIBRARY launches only -- what a command list carries: ``dev_loss += lv`` by
        lirec_scalar_accumulate, ``dev_rels[at:at + bs].copy_(rl)`` by lirec_rows_copy_at at the output cursor (with the batch's labels
        and pair hashes, which the eager loop keeps as views of a buffer per batch: a replayed step has ONE buffer).  Every batch field
        the kernels read must be read IN PLACE from the batch's buffer -- a converted copy would be the recording batch's for every
        replay: raised before anything is accumulated, and the loop stays eager."""
        blob, labels, ints = batch['_dev_blob'], batch['labels'], out['inters']
        bs = labels.shape[0]

        def in_place(t, what):
            t = t.to(ints.device).contiguous()
            if not RecordedEvalStep.in_batch(blob, t):
                raise LirecError('testing(record_eval): %s is not read in place from the batch buffer' % what)
            return t
        lv = loss(out, batch)
        y = in_place(labels.long().reshape(-1), 'labels')
        if on_device:
            Tn = ints.numel() // (bs * ints.shape[-1])
            rels = out['rels'] if opt.ctx == 1 else None
            args = (in_place(batch['mem_mask'].double(), 'mem_mask'), y,
                    in_place(batch['rels_label'].long(), 'rels_label') if rels is not None else None,
                    in_place(batch['gt_tracks'].long(), 'gt_tracks'), in_place(batch['just_zeros'].to(torch.bool), 'just_zeros'))
            ops.scalar_accumulate(dev_loss, lv.detach().reshape(-1)[:1])
            ops.eval_max_tracks(ints.reshape(bs * Tn, -1), rels.reshape(bs * Tn, -1) if rels is not None else None, *args, dev_counters,
                                bs, Tn, ints.shape[-1], rels.shape[-1] if rels is not None else 0, loader_types=True)
            return
        if opt.soft_gt:
            soft = in_place(batch['soft_labels'].double(), 'soft_labels').reshape(bs, -1)
            ops.scalar_accumulate(dev_loss, lv.detach().reshape(-1)[:1])
            ops.eval_clip_topk(ints, y, dev_counters, conf=dev_conf, soft=soft, loader_types=True)
        elif opt.rels_multitask:
            if opt.ctx == 1:
                in_place(batch['rels_label'], 'rels_label'), in_place(batch['hash_rel'], 'hash_rel')
                if batch['rels_label'].dtype != torch.int64 or batch['hash_rel'].dtype != torch.int64:
                    raise LirecError('testing(record_eval): rels_label / hash_rel are kept as int64 rows')
            ops.scalar_accumulate(dev_loss, lv.detach().reshape(-1)[:1])
            ops.eval_clip_topk(ints.reshape(bs, -1, ints.shape[-1])[:, 0], y, dev_counters, conf=dev_conf,
                               y_stride=labels.numel() // bs, loader_types=True)
            if opt.ctx == 1:
                ops.rows_copy_at(out['rels'].detach().reshape(bs, -1), dev_rels, rec['cursor'].word)
                rec['labels'] = keep_rows(batch['rels_label'], rec['labels'])
                rec['hashes'] = keep_rows(batch['hash_rel'], rec['hashes'])
                ops.counter_add(rec['cursor'].word, [bs])
        else:
            if opt.tracks:
                raise LirecError('testing(record_eval): the track count of this recipe is a torch reduction per batch')
            ops.scalar_accumulate(dev_loss, lv.detach().reshape(-1)[:1])
            ops.eval_clip_topk(ints, y, dev_counters, conf=dev_conf, loader_types=True)

    with torch.no_grad():
        for idx, batch in enumerate(loader):
            if stepper is not None and len(batch['labels']) != 1:
                rec['cursor'].expect(rels_at)
                done, batch = stepper.take(batch, recorded_tail, state=[t for t in (dev_counters, dev_loss, dev_conf) if t is not None])
                if done:
                    # (the host's account of a batch the list evaluated: what the two device branches below keep)
                    bs = len(batch['labels'])
                    n_clips, n_batches = n_clips + bs, n_batches + 1
                    if on_device_topk and opt.rels_multitask and not opt.soft_gt and opt.ctx == 1:
                        assert rels_at + bs <= dev_rels.shape[0], 'a block store yields its own length'
                        rels_parts.append((rels_at, bs, None, kept_rows(rec['labels'], batch['rels_label'], rels_at, bs),
                                           kept_rows(rec['hashes'], batch['hash_rel'], rels_at, bs)))
                        rels_at += bs
                        rec['cursor'].advanced(bs)
                    continue
                rec['cursor'].invalidate()        # (an eager batch moves rels_at and not the word; a failed recording may have moved the word)
            if to_dev is not None:
                batch = to_dev(batch)             # (one host-to-device copy for the batch's small tensors; device counters only)
            labels = batch['labels']
            if len(labels) == 1:                      # the reference skips singleton batches (:38-39)
                continue
            out = model(batch)
            if to_dev is None and isinstance(batch, dict) and batch.get('_slots') and getattr(out.get('inters'), 'is_cuda', False):
                # (host-counter path: the model moved the pooled, page-locked tables itself -- hand the buffers back once those
                #  copies are done, or every batch would keep its slots and the pool would grow by a batch per iteration)
                from .features import PinnedPool
                PinnedPool.copied(batch['_slots'])
            lv = loss(out, batch)
            n_clips += len(labels)
            if on_device:
                # counters and loss stay on the GPU; nothing is copied back inside the loop
                ints = out['inters']
                if dev_counters is None:
                    dev_counters = torch.zeros(8, dtype=torch.int64, device=ints.device)
                    dev_loss = torch.zeros(1, dtype=torch.float32, device=ints.device)
                dev_loss += lv.detach().reshape(-1)[:1]
                n_batches += 1
                bs, Tn = labels.shape[0], ints.numel() // (labels.shape[0] * ints.shape[-1])
                dv = lambda t: t.to(ints.device, non_blocking=True).contiguous()
                rels = out['rels'] if opt.ctx == 1 else None
                ops.eval_max_tracks(ints.reshape(bs * Tn, -1), rels.reshape(bs * Tn, -1) if rels is not None else None,
                                    dv(batch['mem_mask'].double()), dv(labels.long().reshape(-1)),
                                    dv(batch['rels_label'].long()) if rels is not None else None,
                                    dv(batch['gt_tracks'].long()), dv(batch['just_zeros'].to(torch.bool)), dev_counters,
                                    bs, Tn, ints.shape[-1], rels.shape[-1] if rels is not None else 0, loader_types=True)
                continue
            if on_device_topk:
                # counters, confusion matrix and loss stay on the GPU, the relationship logits wait there: nothing is copied back
                # inside the loop.  The batch itself stays where the loader left it: its labels go up, a few bytes.
                ints = out['inters']
                if dev_counters is None:
                    dev_counters = torch.zeros(8, dtype=torch.int64, device=ints.device)
                    dev_conf = torch.zeros(conf_mat.shape, dtype=torch.int64, device=ints.device)
                    dev_loss = torch.zeros(1, dtype=torch.float64, device=ints.device)
                dev_loss += lv.detach().reshape(-1)[:1]
                n_batches, n_out = n_batches + 1, len(out)        # sic: the average is weighted by len(output dict) (:42)
                bs = labels.shape[0]
                dv = lambda t: t.to(ints.device, non_blocking=True)
                if opt.soft_gt:
                    ops.eval_clip_topk(ints, dv(labels.long()).reshape(-1), dev_counters, conf=dev_conf,
                                       soft=dv(batch['soft_labels'].double()).reshape(bs, -1), loader_types=True)
                elif opt.rels_multitask:
                    # row 0 of each clip's group of rows and labels[:, 0], both read in place
                    ops.eval_clip_topk(ints.reshape(bs, -1, ints.shape[-1])[:, 0], dv(labels.long()).reshape(-1), dev_counters,
                                       conf=dev_conf, y_stride=labels.numel() // bs, loader_types=True)
                    if opt.ctx == 1:
                        rl = out['rels'].detach().reshape(bs, -1)
                        if dev_rels is None:              # one buffer for the clips this process evaluates
                            n_share = len(sampler.indices()) if sampler is not None else len(test_dataset)
                            dev_rels = torch.empty(max(n_share, bs), rl.shape[1], dtype=rl.dtype, device=rl.device)
                        if rels_at + bs > dev_rels.shape[0]:          # (a dataset that yields more clips than its length)
                            dev_rels = torch.cat([dev_rels, torch.empty_like(dev_rels)])
                        dev_rels[rels_at:rels_at + bs].copy_(rl)
                        if batch['rels_label'].is_cuda:
                            # (a batch made on the device -- lirec_amd.loader.BlockLoader: its labels wait there like the logits)
                            rels_parts.append((rels_at, bs, None, batch['rels_label'], batch['hash_rel']))
                        else:
                            sel = torch.nonzero(batch['rels_label'] - n_rels + 1)         # the loader's host tensors
                            if sel.shape[0]:
                                rels_parts.append((rels_at, bs, sel, batch['rels_label'][sel].squeeze(1), batch['hash_rel'][sel].squeeze(1)))
                        rels_at += bs
                else:
                    if opt.tracks and batch['just_zeros'].is_cuda:
                        dev_tracks = batch['just_zeros'].sum() + (dev_tracks if dev_tracks is not None else 0)   # (read after the loop)
                    elif opt.tracks:
                        total_tracks += int(np.sum(batch['just_zeros'].cpu().numpy()))       # (a host tensor of the loader)
                    ops.eval_clip_topk(ints, dv(labels.long()).reshape(-1), dev_counters, conf=dev_conf, loader_types=True)
                continue
            losses.update(lv.item(), len(out))        # sic: weighted by len(output dict) (:42)
            inters = out['inters'].cpu() if out.get('inters') is not None else None
            if opt.soft_gt:
                conf_mat = prec.update_probs(inters, labels, soft_labels=batch['soft_labels'], conf_mat=conf_mat)
            elif opt.tr_maximize:
                bs = labels.shape[0]
                if opt.ints == 1 and opt.ctx == 0:
                    prec.update_probs_max_tracks(inters.reshape(bs, -1, inters.shape[-1]), gt_tracks=batch['gt_tracks'],
                                                 gt_classes=labels, print_batch=idx == 0, n_names=batch['n_names'],
                                                 mask=batch['mem_mask'].cpu(), just_zeros=batch['just_zeros'])
                if opt.ints == 1 and opt.ctx == 1:
                    rels_mask = torch.nonzero(batch['rels_label'][:, 0] - n_rels + 1)
                    prec.update_probs_max_tracks_rels(inters.reshape(bs, -1, inters.shape[-1]), out['rels'].cpu(),
                                                      labels, batch['rels_label'], gt_tracks=batch['gt_tracks'],
                                                      just_zeros=batch['just_zeros'], mask=batch['mem_mask'].cpu(),
                                                      rels_mask=rels_mask)
            elif opt.rels_multitask:
                if opt.ints == 1:
                    bs = labels.shape[0]
                    conf_mat = prec.update_probs(inters.reshape(bs, -1, inters.shape[-1])[:, 0],
                                                 labels[:, 0].reshape(-1), conf_mat=conf_mat)
                if opt.ctx == 1:
                    sel = torch.nonzero(batch['rels_label'] - n_rels + 1)
                    if sel.shape[0]:
                        prec_rels.update(out['rels'].cpu()[sel].squeeze(1), batch['rels_label'][sel].squeeze(1),
                                         batch['hash_rel'][sel].squeeze(1))
            else:
                if opt.tracks:
                    total_tracks += int(np.sum(batch['just_zeros'].cpu().numpy()))
                conf_mat = prec.update_probs(inters, labels, conf_mat=conf_mat)
    recorded_steps = 0
    if stepper is not None:
        recorded_steps = stepper.replayed
        stepper.close()                                           # (the list lives for this call: parameters change between evaluations)
    if on_device and dev_counters is not None:
        prec.add_device_counters(dev_counters)                    # the only device-to-host copies of the evaluation
        losses.update(float(dev_loss) / max(n_batches, 1), max(n_batches, 1))
    if on_device_topk and dev_counters is not None:
        # the evaluation's device-to-host copies: the counters, the confusion matrix, the loss and the relationship logits
        prec.add_device_topk_counters(dev_counters)
        conf_mat += dev_conf.cpu().numpy()
        losses.val = float(dev_loss) / n_batches
        losses.sum, losses.count = float(dev_loss) * n_out, n_out * n_batches
        losses.avg = losses.sum / losses.count
        if dev_tracks is not None:
            total_tracks += int(dev_tracks)
        if rels_parts:
            rels_host = dev_rels[:rels_at].cpu()
            for at, bs, sel, gt_rel, hashes in rels_parts:            # batch by batch, in order: the host path's sums
                if sel is None:                                       # (device batches: selected here, as the host batches were in the loop)
                    gt_all, hash_all = gt_rel.cpu(), hashes.cpu()
                    sel = torch.nonzero(gt_all - n_rels + 1)
                    if not sel.shape[0]:
                        continue
                    gt_rel, hashes = gt_all[sel].squeeze(1), hash_all[sel].squeeze(1)
                prec_rels.update(rels_host[at:at + bs][sel].squeeze(1), gt_rel, hashes)
    if sharded:
        # the ranks' sums become the dataset's: Precision's counters, the loss average's numerator and denominator, the clip
        # counts -- one small all-reduce -- then the confusion matrix and the per-pair relationship scores
        parallel.reduce_precision(prec)
        tot = parallel.all_reduce_counters({'loss_sum': float(losses.sum), 'loss_count': float(losses.count), 'n_clips': int(n_clips),
                                            'total_tracks': int(total_tracks)})
        losses.sum, losses.count = tot['loss_sum'], tot['loss_count']
        losses.avg = losses.sum / losses.count if losses.count else 0.0
        n_clips, total_tracks = tot['n_clips'], tot['total_tracks']
        conf_mat = parallel.all_reduce_array(conf_mat)
        if prec_rels is not None:
            parallel.merge_relationships(prec_rels)
    dt = time.time() - t0
    say = print if verbose else (lambda *a, **k: None)
    say(prec.total)
    say('tracks # %d' % total_tracks)
    say('%s clips/s: %.1f (%d clips in %.2f s)' % (mode.upper(), n_clips / max(dt, 1e-9), n_clips, dt))

    out_val = out_ints = out_rels = out_tr = out_joint = 0
    if opt.ints == 1:
        say('%s loss: %f' % (mode.upper(), losses.avg))
        say('%s pr@1: %f' % (mode.upper(), prec.top1()))
        if not opt.tr_maximize:
            say('%s pr@5: %f' % (mode.upper(), prec.top5()))
        out_ints = out_joint = prec.top1()
        out_val += out_ints
    if opt.soft_gt:
        say('%s pr soft@1 %f' % (mode.upper(), prec.top1_sf()))
        say('%s pr soft@5 %f' % (mode.upper(), prec.top5_sf()))
    if opt.tr_maximize:
        out_ints, out_tr = prec.cls_top1(), prec.trks_top1()
        out_val = out_val + out_tr + out_ints
        say('%s pr@trks: %f' % (mode.upper(), out_tr))
        say('%s pr@cls: %f' % (mode.upper(), out_ints))
        if opt.ctx == 1:
            out_rels = prec.rels_top1()
            say('%s pr@rels: %f' % (mode.upper(), out_rels))
            out_val += out_rels
    if opt.rels_multitask and opt.ctx == 1 and not opt.tr_maximize:
        out_rels = prec_rels.top1() if prec_rels._gt else 0.0
        out_val += out_rels
        say('%s rels@top1: %f' % (mode.upper(), out_rels))
        say('%s rels@top3: %f' % (mode.upper(), prec_rels.top3() if prec_rels._gt else 0.0))
        say('%s rel+int: %f' % (mode.upper(), out_val))

    out = {'total': out_val, 'ints': out_ints}
    testing.last = {'precision': prec, 'relationships': prec_rels, 'conf_mat': conf_mat, 'loss': losses.avg, 'n_clips': n_clips,
                    'metrics_on_device': bool(on_device or on_device_topk), 'recorded_steps': recorded_steps}
    if opt.rels_multitask:
        out['rels'] = out_rels
    if opt.tr_maximize:
        out.update({'tracks': out_tr, 'joint': out_joint})
    return out


def clip_losses(dataset, model, loss, batch_size=None):
    """The loss of every clip of ``dataset``: float32 numpy ``[n, 2]`` in dataset order, columns (lymbda * interaction term,
    relationship term) -- the per-clip values of the loss kernel (``lirec_clip_weights::clip_loss``), UNWEIGHTED and undivided,
    whatever weights the dataset carries.  What hard-example mining, label-noise triage or a curriculum rank the clips by.
    Eval mode, no gradients, the loader selection of ``testing()``; singleton batches are NOT skipped (every clip gets its row); the
    values stay on the device until ONE copy at the end.  The model's mode and ``loss.keep_clip_losses`` are restored."""
    bs = int(batch_size or opt.batch_size)
    loader = make_loader(dataset, bs)
    was_training, kept = model.training, loss.keep_clip_losses
    model.eval()
    loss.keep_clip_losses = True
    parts = []
    try:
        with torch.no_grad():
            to_dev = getattr(dataset, 'to_device', None) if str(opt.device).startswith('cuda') else None
            for batch in loader:
                if to_dev is not None:
                    batch = to_dev(batch)
                loss(model(batch), batch)
                parts.append(loss.last_clip_losses)
    finally:
        loss.keep_clip_losses = kept
        loss.last_clip_losses = None
        model.train(was_training)
    if not parts:
        return np.zeros((0, 2), dtype=np.float32)
    return torch.cat(parts).cpu().numpy()
