"""Gradient accumulation through the real Python host stack in the library's host-side DRY RUN (tests/host_dryrun.py) -- the driver
of tests/test_host_accum.py, run in a process of its own (the dry run patches torch and switches the library process-wide); not
a test module.  What is looked at is what the host ISSUES: the calls of lirec_amd.ops that stand for launches, in order, each with
whether it was issued under ``ops.adam_hold``; the recorded command lists; and the host's books (phase, step, state_dict)."""
import sys

import host_dryrun as H
import accum_cases as XC

import torch  # noqa: E402

from lirec_amd import _lib, config, ops  # noqa: E402
from lirec_amd import model as M  # noqa: E402
from lirec_amd._lib import LirecError  # noqa: E402
from lirec_amd.config import opt  # noqa: E402
from lirec_amd.graph import RecordedTrainStep  # noqa: E402
from lirec_amd.optim import FusedAdam  # noqa: E402

SMALL = dict(text_dim=24, visual_dim=32, track_dim=32, joint_dim=16)
RECIPES = {'int_rel_ch': (11, 5, 4, 4, 3), 'int_rels': (11, 5, 5, 1, 3), 'int_ch': (11, 5, 4, 4, 0), 'modalties': (11, 0, 6, 1, 0)}
ADAM = ('adam_step', 'adam_step_counted', 'adam_step_ranges', 'adam_step_groups')
ZEROING = ('zero_', 'zero_count')
LOGGED = ADAM + ZEROING + ('counter_add', 'accum_begin', 'ema_step', 'fused_adam_args')

LOG, HELD = [], [False]


def spy():
    """every logged op appends (name, issued under adam_hold?); CommandList.begin appends a marker"""
    for name in LOGGED:
        fn = getattr(ops, name)

        def wrapped(*a, _fn=fn, _name=name, **kw):
            LOG.append((_name, HELD[0]))
            return _fn(*a, **kw)
        setattr(ops, name, wrapped)
    enter, leave = ops.adam_hold.__enter__, ops.adam_hold.__exit__

    def on(self):
        HELD[0] = self.hold is not None
        return enter(self)

    def off(self, *exc):
        HELD[0] = False
        return leave(self, *exc)
    ops.adam_hold.__enter__, ops.adam_hold.__exit__ = on, off
    begin = ops.CommandList.begin

    def marked(*a, **kw):
        LOG.append(('RECORD', False))
        return begin(*a, **kw)
    ops.CommandList.begin = staticmethod(marked)


def make(kind, seed=3, **flags):
    from lirec_amd.data import synthetic_batch
    n_classes, n_rels, B, T, R = RECIPES[kind]
    config.reset()
    config.recipe(kind, dropout=0.3, dropout_seed=5, **SMALL, **({} if kind in ('int_ch', 'modalties') else {'rels_n_clips': R}))
    opt.device = 'cpu'
    opt.wgrad_side_stream = False
    for k, v in flags.items():
        setattr(opt, k, v)
    model, loss, optim = M.create_model(n_classes, n_rels=n_rels)
    model.train()
    kw = dict(n_classes=n_classes, n_rels=n_rels, **{k: v for k, v in SMALL.items() if k != 'joint_dim'})
    if kind in ('int_ch', 'int_rel_ch'):
        kw['T'] = T
    if kind in ('int_rels', 'int_rel_ch'):
        kw['R'] = R
    hb = synthetic_batch(seed, kind, B, **kw)
    batch = {k: (v.float() if (torch.is_tensor(v) and k == 'features') else v) for k, v in hb.items()}
    return model, loss, optim, batch


def eager(model, loss, optim, batch):
    optim.zero_grad()
    lv = loss(model(dict(batch)), batch)
    lv.backward()
    optim.step()


def names(entries):
    return [n for n, _ in entries]


def steps_of(optim):
    sd = optim.state_dict()
    return sorted({int(sd['state'][i]['step']) for i in sd['state']})


def eager_chain():
    """the stock loop over a chain of calls with k changing between windows: zeroing exactly where a window opens, Adam launches
    exactly on apply calls, step = updates, the phase as restated"""
    model, loss, optim, batch = make('int_rel_ch')
    assert optim.accumulate_steps == 1 and optim.accum_phase == 0
    model.flat_grads(attach=True)                 # (the buffer exists from the first zero_grad() on)
    ks = [2, 2, 2, 2, 3, 3, 3, 1, 2, 2, 3]
    want = XC.chain(ks)
    for call, (k, (phase, zeroes, applies, updates)) in enumerate(zip(ks, want)):
        if phase == 0:
            optim.accumulate_steps = k
        else:
            try:
                optim.accumulate_steps = k + 1
                raise AssertionError('a change of k inside a window was accepted')
            except RuntimeError as e:
                assert 'middle of a window' in str(e)
        assert optim.accum_phase == phase, (call, optim.accum_phase, phase)
        del LOG[:]
        eager(model, loss, optim, batch)
        got = names(LOG)
        assert any(n in ZEROING for n in got) == zeroes, (call, got)
        assert any(n in ADAM for n in got) == applies, (call, got)
        assert 'accum_begin' not in got and not any(h for _, h in LOG), (call, 'the eager loop decides on the host')
        assert optim._step == updates and steps_of(optim) == ([updates] if updates else [0]), (call, optim._step, updates)
    assert optim.accum_phase == 1                 # (the chain ends inside a window of three)
    optim.drop_window()
    assert optim.accum_phase == 0
    for bad in (0, -1, 2.0, True, None, '2'):
        try:
            optim.accumulate_steps = bad
            raise AssertionError('accumulate_steps = %r was accepted' % (bad,))
        except ValueError:
            pass
    assert optim.arm_first_layer_update() in (False,)          # (k = 3: never folded)
    print('eager chain ok')


def _variant(name, k):
    if name == 'ema':
        model, loss, optim, batch = make('int_rel_ch', ema_decay=0.9)
    elif name == 'adamw':
        model, loss, optim, batch = make('int_rel_ch')
        optim = FusedAdam(model, lr=1e-3, weight_decay=1e-2, device_hyper=True, decoupled_weight_decay=True)
    else:
        model, loss, optim, batch = make('int_rel_ch')
    if name == 'frozen':
        next(p for n, p in model.named_parameters() if n.endswith('.weight')).requires_grad_(False)
    optim.accumulate_steps = k
    return model, loss, optim, batch


def recorded_sequences():
    """the accumulating recorded step: the head launch first, no zeroing / counter launch, no folded update, every Adam / EMA
    launch under the hold; recorded at phase 0 and 1; the host's books over replays, an eager step in between, release / resume"""
    for name in ('plain', 'ema', 'adamw', 'frozen'):
        for k, phase0 in ((2, 0), (2, 1), (3, 1), (3, 2)):
            model, loss, optim, batch = _variant(name, k)
            for _ in range(phase0):
                eager(model, loss, optim, batch)
            assert optim.accum_phase == phase0 and optim._step == 0
            del LOG[:]
            g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
            at = names(LOG).index('RECORD')
            rec = LOG[at + 1:]
            got = names(rec)
            assert got[0] == 'accum_begin' and got.count('accum_begin') == 1, (name, k, got)
            assert not any(n in ZEROING + ('counter_add', 'fused_adam_args') for n in got), (name, k, got)
            upd = [(n, h) for n, h in rec if n in ADAM + ('ema_step',)]
            assert upd and all(h for _, h in upd), (name, k, rec)
            assert any(n in ADAM for n, _ in upd) and (name != 'ema' or any(n == 'ema_step' for n, _ in upd)), (name, upd)
            assert (g.overwrite, g.fused, g.defer) == (False, False, False) and g.accum == k
            assert optim._win_dev is g.win and g.hyper_key(optim)[-1] == ('accumulate_steps', k)
            calls = phase0 + 2                                    # (the warm-up step and the recording step were real micro-steps)
            for _ in range(2 * k + 1):
                g.step()
                calls += 1
                assert optim.accum_phase == calls % k and optim._step == calls // k, (name, k, calls, optim.accum_phase, optim._step)
            g.release()
            assert optim._win_dev is None and optim._step_dev is None
            del LOG[:]
            eager(model, loss, optim, batch)                      # (continues the same window, decided on the host)
            calls += 1
            assert optim.accum_phase == calls % k and optim._step == calls // k
            assert any(n in ADAM for n in names(LOG)) == (calls % k == 0) and not any(h for _, h in LOG)
            g.resume()
            assert optim._win_dev is g.win
            g.step()
            calls += 1
            assert optim.accum_phase == calls % k and optim._step == calls // k and steps_of(optim)[-1] == calls // k      # (a frozen parameter: 0)
            optim.accumulate_steps = k                            # (the same value: fine while recorded)
            if optim.accum_phase == 0:
                try:
                    optim.accumulate_steps = k + 1
                    raise AssertionError('k changed under a recorded step')
                except RuntimeError as e:
                    assert 'release' in str(e)
            g.release()
            g.cmds.destroy()
    print('recorded sequences ok')


def refusals():
    model, loss, optim, batch = make('int_rel_ch')
    optim.accumulate_steps = 2
    for kw, word in ((dict(max_grad_norm=1.0), 'max_grad_norm'), (dict(skip_nonfinite=True), 'skip_nonfinite')):
        for a, v in kw.items():
            setattr(optim, a, v)
        try:
            RecordedTrainStep(model, loss, optim, batch, warmup=1)
            raise AssertionError('recorded accumulation with %s was not refused' % word)
        except LirecError as e:
            assert word in str(e) and 'accumulation' in str(e)
        optim.max_grad_norm, optim.skip_nonfinite = None, False
        assert optim._win_dev is None and optim._step_dev is None and optim.accum_phase == 0
    try:
        RecordedTrainStep(model, loss, optim, batch, warmup=1, next_batch=dict(batch))
        raise AssertionError('the input-pipeline form with accumulation was not refused')
    except LirecError as e:
        assert 'accumulation' in str(e)
    print('refusals ok')


def off_is_off():
    """accumulate_steps = 1, by keyword or by assignment, against an optimiser of THIS tree built without it: the same ops in the
    same order over two eager steps, and the same recorded commands on the same streams.  (No sequence of the parent commit is
    stored anywhere to compare with: that the k = 1 sequences are the parent's is what the untouched tests/test_host_embed_heads.py
    and the other existing launch-sequence tests hold, and what profiles/accum_steps.json counts -- 73 recorded commands in both.)"""
    for kind in RECIPES:
        seqs = []
        for how in ('without', 'keyword', 'assigned'):
            model, loss, optim, batch = make(kind)
            if how == 'keyword':
                g0 = optim.param_groups[0]
                optim = FusedAdam(model, lr=g0['lr'], weight_decay=g0['weight_decay'], accumulate_steps=1)
            elif how == 'assigned':
                optim.accumulate_steps = 1
            del LOG[:]
            eager(model, loss, optim, batch)
            eager(model, loss, optim, batch)
            cmds, flags = None, None
            if kind != 'modalties':
                g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
                lanes = {}
                cmds = [(lanes.setdefault(s, len(lanes)), k) for s, k in (g.cmds.command(i) for i in range(g.cmds.size))]
                flags = (g.overwrite, g.fused, g.defer, g.hyper_key(optim))
                g.step()
                g.release()
                g.cmds.destroy()
            assert 'accum_begin' not in names(LOG) and not any(h for _, h in LOG)
            seqs.append((list(LOG), cmds, flags, optim._step, optim.accum_phase))
        assert seqs[0] == seqs[1] == seqs[2], (kind, [len(s[0]) for s in seqs])
        assert seqs[0][0] and seqs[0][4] == 0
    print('off is off ok')


def main(what):
    L = _lib.lib()
    assert L.lirec_debug_set(H.DRY, -1) == 0
    H.patch()
    spy()
    ops.set_gemm_mode(2)
    {'eager_chain': eager_chain, 'recorded_sequences': recorded_sequences, 'refusals': refusals, 'off_is_off': off_is_off}[what]()
    config.reset()
    assert L.lirec_debug_set(0, -1) == 0


if __name__ == '__main__':
    main(sys.argv[1])
