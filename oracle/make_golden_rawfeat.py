#!/usr/bin/env python
"""Golden vectors for the raw-feature pooling, produced by the REFERENCE's own feature classes.

Build-container only.  ``VisualFeatures`` and ``TextFeatures`` read MovieGraphs files in ``__init__``; instances are
made with ``__new__`` and given the arrays those files would hold (a synthetic I3D grid, frame <-> second table, token
matrix, dialog times).  What computes is the reference: ``VisualFeatures.get_features_by_time`` /
``get_features_by_track`` (visual_utils/visual_features.py:60-143, opt.tf_crop), ``TextFeatures.second_to_last`` and
``get_features_by_time`` (text_utils/text_features.py:140-182), followed by ``np.max(axis=0, keepdims=True)`` -- the
``f_visual`` / ``f_text`` of mixed_utils/mixed_features.py:37-38,54,61,104-105 (MixedFeatures itself writes its results
into a cache directory under the data root, so its two lines are applied here instead of calling it).
Writes tests/golden/rawfeat.npz: inputs + the reference's outputs, and tests/golden/rawfeat_edges.npz: a second, smaller scene
made of the bookkeeping's edges (``scene_edges``).  An output directory may be given as the only argument.
"""
import contextlib
import io
import os
import sys
import types
import warnings
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
REF = '/root/reference'
OUT = os.path.join(ROOT, 'tests', 'golden')


def load_reference():
    argv = sys.argv
    sys.argv = ['oracle']
    sys.path.insert(0, REF)
    bert = types.ModuleType('pytorch_pretrained_bert')
    bert.BertTokenizer = bert.BertModel = bert.BertForMaskedLM = object
    sys.modules.setdefault('pytorch_pretrained_bert', bert)
    from utils.arg_pars import opt
    with contextlib.redirect_stdout(io.StringIO()):
        import visual_utils.visual_features as VF
        import text_utils.text_features as TF
    sys.argv = argv
    return opt, VF, TF


f_max = lambda a: np.max(a, axis=0, keepdims=True)                  # mixed_features.py:37-38


def scene_one(opt, VF, TF, out_dir):
    rng = np.random.Generator(np.random.PCG64(11))
    F, Cc, H, W = 9, 24, 13, 15                       # 13 x 15 = 195 cells: above numpy's 128-element pairwise block
    opt.visual_dim, opt.text_dim, opt.tf_crop, opt.spat_pool, opt.sampling_fr = Cc, 12, True, True, 0.0625
    opt.contextualization = 'second-to-last'
    grid = np.maximum(rng.standard_normal((F, Cc, H, W)), 0).astype(np.float32)
    vf = VF.VisualFeatures.__new__(VF.VisualFeatures)
    vf.features, vf.dims = grid, (480, 720)           # original resolution (height, width), load_orig_resol()
    vf.frame2time, vf.time2frame = {}, defaultdict(list)
    for frame in range(0, F * 16 + 8):                # original frames at 16 per grid step, 24 per second
        sec = frame // 24
        vf.frame2time[frame] = sec
        vf.time2frame[sec].append(frame)
    secs = max(vf.time2frame)
    time_nodes = [{'start': 0, 'end': 1}, {'start': 1, 'end': 3}, {'start': 2, 'end': secs + 1}, {'start': 3, 'end': secs}]
    fx = {'grid': grid, 'dims': np.array(vf.dims), 'sampling_fr': np.array(opt.sampling_fr),
          'frame2time': np.array([vf.frame2time[k] for k in sorted(vf.frame2time)]),
          'time_nodes': np.array([[t['start'], t['end']] for t in time_nodes])}
    clip = [f_max(vf.get_features_by_time(t)) for t in time_nodes]               # :54
    fx['clip_visual'] = np.concatenate(clip).astype(np.float32)
    assert np.array_equal(fx['clip_visual'].astype(np.float64), np.concatenate(clip))
    # tracks: face boxes at original resolution x 2 (the reference halves them, :118), some partly / wholly off the grid,
    # one element at the frame index the reference skips, one track with an empty crop
    tracks = []
    for k in range(6):
        tr = []
        for _ in range(int(rng.integers(1, 6))):
            tr.append({'frame': int(rng.integers(0, F * 16)), 'x': float(rng.uniform(0, 1300)), 'y': float(rng.uniform(0, 900)),
                       'w': float(rng.uniform(40, 300)), 'h': float(rng.uniform(40, 300))})
        tracks.append(tr)
    tracks[1].append({'frame': F * 16, 'x': 100.0, 'y': 100.0, 'w': 80.0, 'h': 80.0})          # int(F*16/16) == F -> skipped
    tracks[4] = [{'frame': 16, 'x': 5000.0, 'y': 100.0, 'w': 60.0, 'h': 60.0}]                 # box right of the grid: empty crop
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tr in tracks:
            outs.append(f_max(vf.get_features_by_track(tr)))                                   # :104-105
    fx['track'] = np.concatenate(outs).astype(np.float32)
    fx['n_tracks'] = len(tracks)
    for k, tr in enumerate(tracks):
        fx['track/%d' % k] = np.array([[e['frame'], e['x'], e['y'], e['w'], e['h']] for e in tr], dtype=np.float64)
    # text
    n_tok, layers = 40, 4
    tf = TF.TextFeatures.__new__(TF.TextFeatures)
    tf.video_idx, tf.scene_idx, tf._n = 'tt', '000', 4
    raw = rng.standard_normal((n_tok, layers, opt.text_dim)).astype(np.float32)
    tf.features = raw.copy()
    tf.second_to_last()                                                                        # :181-182
    bounds = [0, 7, 15, 22, 31, 40]
    tf.time_idx2token_range = [list(range(bounds[i], bounds[i + 1])) for i in range(5)]
    dial = [(0, 1), (2, 2), (3, 5), (6, 6), (9, 12)]
    tf.times = [TF.Time(a, b) for a, b in dial]
    tf.dialogs = [''] * 5
    tnodes = [{'start': 0, 'end': 2}, {'start': 4, 'end': 4}, {'start': 7, 'end': 8}, {'start': 5, 'end': 10}]
    with contextlib.redirect_stdout(io.StringIO()):
        txt = [f_max(tf.get_features_by_time(t)).reshape(1, -1) for t in tnodes]               # :61-62
    fx.update(tokens=raw, token_bounds=np.array(bounds), dialog_times=np.array(dial), text_time_nodes=np.array([[t['start'], t['end']] for t in tnodes]),
              clip_text=np.concatenate(txt).astype(np.float32))
    np.savez_compressed(os.path.join(out_dir, 'rawfeat.npz'), **fx)
    print('rawfeat fixture: clip_visual %s track %s (NaN rows: %d) clip_text %s' % (
        fx['clip_visual'].shape, fx['track'].shape, int(np.isnan(fx['track']).any(1).sum()), fx['clip_text'].shape))


def scene_edges(opt, VF, TF, out_dir):
    """The bookkeeping's edges, each by construction (the random scene above meets none of them): face boxes whose person box ends
    LEFT of / ABOVE the frame -- the upper bound of the reference's slice is then negative and numpy counts it from the far end
    (visual_features.py:127-133) --, boxes over each border, one cell, the whole grid, a skipped element; clips on the ``end - 1``
    rule, past the grid's end, with start == end; dialog lines that meet each clause of ``Time.includes`` alone."""
    rng = np.random.Generator(np.random.PCG64(23))
    F, Cc, H, W = 4, 16, 13, 15
    opt.visual_dim, opt.text_dim, opt.tf_crop, opt.spat_pool, opt.sampling_fr = Cc, 8, True, True, 0.0625
    opt.contextualization = 'second-to-last'
    grid = rng.standard_normal((F, Cc, H, W)).astype(np.float32)                 # (signed: all-negative means occur)
    vf = VF.VisualFeatures.__new__(VF.VisualFeatures)
    vf.features, vf.dims = grid, (480, 720)
    vf.frame2time, vf.time2frame = {}, defaultdict(list)
    for frame in range(0, 80):                        # seconds 0, 1 and 3: second 2 is missing from the table; grid steps 0 .. 4
        sec = frame // 24 if frame < 48 else 3
        vf.frame2time[frame] = sec
        vf.time2frame[sec].append(frame)
    time_nodes = [{'start': 0, 'end': 2},             # end second missing -> second 1, last grid step 2 < F
                  {'start': 1, 'end': 3},             # end step 4 >= F: up to the grid's end
                  {'start': 1, 'end': 1},             # start == end
                  {'start': 3, 'end': 4},             # both
                  {'start': 0, 'end': 0}]
    fx = {'grid': grid, 'dims': np.array(vf.dims), 'sampling_fr': np.array(opt.sampling_fr),
          'frame2time': np.array([vf.frame2time[k] for k in sorted(vf.frame2time)]),
          'time_nodes': np.array([[t['start'], t['end']] for t in time_nodes])}
    clip = [f_max(vf.get_features_by_time(t)) for t in time_nodes]
    fx['clip_visual'] = np.concatenate(clip).astype(np.float32)
    assert np.array_equal(fx['clip_visual'].astype(np.float64), np.concatenate(clip))
    el = lambda frame, x, y, w, h: {'frame': frame, 'x': float(x), 'y': float(y), 'w': float(w), 'h': float(h)}
    tracks = [
        [el(16, -400, 100, 40, 60)],                                             # left of the frame: columns 0:-3
        [el(32, 300, -600, 40, 60)],                                             # above it: rows 0:-3
        [el(48, -400, -600, 40, 60), el(5, 600, 300, 120, 90)],                  # both, beside an interior box
        [el(0, -20, 200, 80, 60), el(17, 1400, 200, 80, 60), el(33, 600, -20, 80, 60), el(63, 600, 900, 80, 60)],   # the four borders
        [el(20, 511, 308, 10, 8)],                                               # one cell
        [el(40, 0, 0, 2000, 400), el(F * 16, 100, 100, 80, 80)],                 # the whole grid; int(F*16/16) == F -> skipped
        [el(16, -2000, 100, 40, 60)],                                            # so far left that 0:-19 is empty: NaN
        [el(F * 16, 100, 100, 80, 80)],                                          # nothing but a skipped element: zeros
    ]
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tr in tracks:
            outs.append(f_max(vf.get_features_by_track(tr)))
    fx['track'] = np.concatenate(outs).astype(np.float32)
    fx['n_tracks'] = len(tracks)
    for k, tr in enumerate(tracks):
        fx['track/%d' % k] = np.array([[e['frame'], e['x'], e['y'], e['w'], e['h']] for e in tr], dtype=np.float64)
    n_tok, layers = 20, 3
    tf = TF.TextFeatures.__new__(TF.TextFeatures)
    tf.video_idx, tf.scene_idx, tf._n = 'tt', '001', 4
    raw = rng.standard_normal((n_tok, layers, opt.text_dim)).astype(np.float32)
    tf.features = raw.copy()
    tf.second_to_last()
    bounds = [0, 6, 13, 20]
    tf.time_idx2token_range = [list(range(bounds[i], bounds[i + 1])) for i in range(3)]
    dial = [(2, 5), (10, 12), (14, 14)]
    tf.times = [TF.Time(a, b) for a, b in dial]
    tf.dialogs = [''] * 3
    tnodes = [{'start': 4, 'end': 9},                 # line 0 by "start inside the line" alone
              {'start': 0, 'end': 3},                 # line 0 by "end inside the line" alone
              {'start': 1, 'end': 8},                 # line 0 by "the clip covers the line" alone
              {'start': 6, 'end': 9},                 # no dialog
              {'start': 11, 'end': 14}]               # lines 1 and 2, each by another clause
    with contextlib.redirect_stdout(io.StringIO()):
        txt = [f_max(tf.get_features_by_time(t)).reshape(1, -1) for t in tnodes]
    fx.update(tokens=raw, token_bounds=np.array(bounds), dialog_times=np.array(dial), text_time_nodes=np.array([[t['start'], t['end']] for t in tnodes]),
              clip_text=np.concatenate(txt).astype(np.float32))
    np.savez_compressed(os.path.join(out_dir, 'rawfeat_edges.npz'), **fx)
    print('rawfeat_edges fixture: clip_visual %s track %s (NaN rows: %d) clip_text %s' % (
        fx['clip_visual'].shape, fx['track'].shape, int(np.isnan(fx['track']).any(1).sum()), fx['clip_text'].shape))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else OUT
    opt, VF, TF = load_reference()
    scene_one(opt, VF, TF, out_dir)
    scene_edges(opt, VF, TF, out_dir)


if __name__ == '__main__':
    main()
