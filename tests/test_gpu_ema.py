"""The exponential moving average of the weights on the device (include/lirec_hip.h, "exponential moving average of the weights";
lirec_amd/optim.py): lirec_ema_step against CPU ``torch.lerp`` and FusedAdam(ema_decay=...) on its eager and recorded routes.

Bounds: none.  One update is fmaf(w, fl32(p - e), e) with w the fp32 rounding of 1 - decay, which is what ``torch.lerp(e, p, w)``
computes on the CPU for w < 0.5, so every comparison of a shadow is by BITS against the chain of CPU lerps over snapshots of the
parameters.  With the average on, parameters and moments are compared by bits with the same run with it off: the lerp launches
read the parameters and write the shadow only.

Measured on an MI355X: zero differing elements in every comparison of this file (kernel: every size, offset, decay and special
value against CPU torch.lerp; FusedAdam: every route and step; recorded against eager over seven steps, with and without an
ema_weights() swap in between); a recorded step at this shape gains three launches, one of them on the side stream.

The models are the small ones of tests/test_gpu_clip.py (18 431 616 flat elements: the side stream's bucket, the middle stretch
and the folded first-layer range are all there), 4 to 7 steps.
"""
import numpy as np
import pytest
import torch

import adamw_cases as WC
import test_gpu_clip as TC
from lirec_amd import _lib, config, ops
from lirec_amd.config import opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 64
CANARY = 1e30
DECAY = 0.9
CAP = _lib.EMA_MAX_BLOCKS


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# 1 - 2. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
DENORMAL = float(np.float32(1e-40))
# (e, p): signed zeros both ways, a denormal shadow, a denormal difference, e == p (a normal, a denormal, a zero), a large ratio
SPECIAL = [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (DENORMAL, 0.0), (0.0, DENORMAL), (1.5, 1.5), (DENORMAL, DENORMAL), (0.0, 0.0),
           (3.0, -0.0), (1.0, 1.0 + 2.0 ** -23), (-1e30, 1e-30), (1e-38, 1.0000001e-38)]
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CAP * 1024 + 3]     # the last: the grid-stride loop runs twice, with a ragged tail


def _values(n, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n).astype(np.float32)
    p = (e + rng.standard_normal(n).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    if n >= 4:
        p[n // 2] = e[n // 2]                                # e == p somewhere in every size
    for i, (a, b) in enumerate(SPECIAL):
        # (at the front, and again at the back: head, body and tail all see them; the small sizes take a rotating few)
        for at in ((i + seed) % n, n - 1 - ((i + seed) % n)) if n < 2 * len(SPECIAL) else (i, n - 1 - i):
            e[at], p[at] = np.float32(a), np.float32(b)
    return torch.from_numpy(e), torch.from_numpy(p)


def _padded(x, off):
    """x at `off` elements behind a 256-byte aligned base + PAD, canaries on both sides"""
    buf = torch.full((PAD + off + x.numel() + PAD,), CANARY, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[PAD + off:PAD + off + x.numel()] = x.to(DEV)
    return buf, buf[PAD + off:PAD + off + x.numel()]


def _outside_ok(buf, off, n):
    return bool((buf[:PAD + off] == CANARY).all()) and bool((buf[PAD + off + n:] == CANARY).all())


@pytest.mark.parametrize('off', [0, 1, 2, 3])
@pytest.mark.parametrize('n', SIZES)
def test_kernel_bits_against_cpu_lerp(n, off):
    for decay in (0.9, 0.9999):
        w = ops.ema_weight(decay)
        e, p = _values(n, 7 * n + off)
        want = torch.lerp(e, p, w)
        ebuf, ev = _padded(e, off)
        pbuf, pv = _padded(p, off)
        assert ev.data_ptr() % 16 == 4 * off and pv.data_ptr() % 16 == 4 * off
        ops.ema_step(ev, pv, w)
        torch.cuda.synchronize()
        diff = int((_bits(ev) != _bits(want)).sum())
        assert diff == 0, (n, off, decay, diff, torch.nonzero(_bits(ev) != _bits(want)).reshape(-1)[:8].tolist())
        assert _outside_ok(ebuf, off, n) and _outside_ok(pbuf, off, n), 'written outside [0, n)'
        assert _same(pv, p), 'the parameters were written'
        # e == p keeps its bits -- but for e = -0, which fmaf(w, +0, -0) = +0 turns into +0 here as in torch (-0 - -0 is +0)
        same = (e == p) & ~((e == 0) & torch.signbit(e))
        assert int(same.sum()) >= 3 or n < 2 * len(SPECIAL)
        assert _same(ev[same.to(DEV)], e[same]), 'e == p did not keep its bits'
        zeros = (e == 0) & (p == 0)
        assert bool((ev[zeros.to(DEV)].cpu().view(torch.int32) == 0).all()), 'zeros in both buffers did not give +0'


def test_a_second_update_continues_the_chain():
    n, w = 4099, ops.ema_weight(DECAY)
    e, p = _values(n, 3)
    _, ev = _padded(e, 1)
    _, pv = _padded(p, 1)
    want = e
    for k in range(3):
        ops.ema_step(ev, pv, w)
        want = torch.lerp(want, p, w)
        pv.add_(0.25)
        p = p + 0.25
    torch.cuda.synchronize()
    assert _same(ev, want)


@pytest.mark.parametrize('n,off', [(5, 3), (1025, 1), (CAP * 1024 + 3, 2)])
def test_the_guard(n, off):
    """flag 0: the bits of the unguarded launch.  Flag 1: the shadow keeps its bits and p is not read -- a NaN in p does not
    reach e (with the flag clear it would: the same launch shows it)"""
    w = ops.ema_weight(DECAY)
    e, p = _values(n, 11)
    _, plain = _padded(e, off)
    _, pv = _padded(p, off)
    ops.ema_step(plain, pv, w)
    guard = torch.tensor([0.37, 2.0, 0.0, CANARY], dtype=torch.float32, device=DEV)
    gbuf, got = _padded(e, off)
    ops.ema_step(got, pv, w, guard=guard)
    torch.cuda.synchronize()
    assert _same(got, plain) and _same(got, torch.lerp(e, p, w)) and _outside_ok(gbuf, off, n)
    assert guard.cpu().tolist() == [np.float32(0.37), 2.0, 0.0, np.float32(CANARY)], 'the guard block was written'
    poisoned = p.clone()
    poisoned[0] = poisoned[n // 2] = poisoned[n - 1] = float('nan')
    _, nv = _padded(poisoned, off)
    guard[2] = 1.0
    sbuf, skipped = _padded(e, off)
    ops.ema_step(skipped, nv, w, guard=guard)
    torch.cuda.synchronize()
    assert _same(skipped, e) and _outside_ok(sbuf, off, n), 'a skipped step changed the shadow'
    guard[2] = 0.0
    ops.ema_step(skipped, nv, w, guard=guard)
    torch.cuda.synchronize()
    assert int(torch.isnan(skipped).sum()) == len({0, n // 2, n - 1})


# ---------------------------------------------------------------------------------------------------------------------------
# 3. FusedAdam(ema_decay=0.9) on every eager route
# ---------------------------------------------------------------------------------------------------------------------------
ROUTES = ['side', 'plain', 'clipped', 'groups', 'frozen']
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        try:
            _cache[key] = fn()
        except BaseException as e:
            _cache[key] = e
    if isinstance(_cache[key], BaseException):
        raise _cache[key]
    return _cache[key]


def _frozen_names(model):
    """a second-layer weight (the middle stretch), a head's bias (the side stream's bucket) and a first-layer weight"""
    from lirec_amd.parallel import stage_of
    names = list(model._offsets)
    pick = [next(n for n in names if stage_of(n) == s and n.endswith(e)) for s, e in ((1, '.weight'), (0, '.bias'), (2, '.weight'))]
    return pick


def _build(route, ema, bound=None):
    from lirec_amd.optim import FusedAdam
    model, loss, optim, batch = TC._fresh(side=route != 'plain')
    if route == 'groups':
        optim = FusedAdam(model, lr=TC.LR, param_groups=WC.two_groups(model), device_hyper=True, ema_decay=ema)
    else:
        optim.ema_decay = ema
    if route == 'clipped':
        optim.max_grad_norm = bound
    return model, loss, optim, batch


def _eager(route, ema, steps=4):
    """[(parameters, m, v, shadow or None) on the host after each step], the shadow at the start, the lerps counted"""
    try:
        # (clipped: half of the first step's gradient norm, so that the coefficient is below 1)
        model, loss, optim, batch = _build(route, ema, TC._clip_bound() if route == 'clipped' else None)
        pd = dict(model.named_parameters())
        out = {'steps': [], 'updates': [], 'coefs': []}
        for s in range(1, steps + 1):
            if route == 'frozen':
                for n in _frozen_names(model):
                    pd[n].requires_grad_(s > 2)                # frozen for two steps, then trained
            TC._backward(model, loss, optim, batch)
            if s == 1:
                out['start'] = None if optim.ema is None else optim.ema.cpu()
                out['p0'] = model.flat_params().cpu()
            optim.step()
            torch.cuda.synchronize()
            out['steps'].append(tuple(t.cpu() for t in TC._state(model, optim)) + (None if optim.ema is None else optim.ema.cpu(),))
            out['updates'].append(optim.ema_updates())
            if route == 'clipped':
                out['coefs'].append(float(optim.clip_coef))
        out['frozen'] = [model._offsets[n] for n in _frozen_names(model)]
        return out
    finally:
        config.reset()


@pytest.mark.parametrize('route', ROUTES)
def test_fused_adam_keeps_the_average_on_every_route(route):
    on = _cached(('eager', route, DECAY), lambda: _eager(route, DECAY))
    off = _cached(('eager', route, None), lambda: _eager(route, None))
    w = ops.ema_weight(DECAY)
    assert _same(on['start'], on['p0']), 'the shadow does not start as a copy of the parameters'
    assert off['start'] is None and all(s[3] is None for s in off['steps']), 'a shadow was made with the average off'
    chain = on['start']
    for s, (a, b) in enumerate(zip(on['steps'], off['steps']), 1):
        chain = torch.lerp(chain, a[0], w)
        diff = int((_bits(a[3]) != _bits(chain)).sum())
        assert diff == 0, (route, s, 'shadow elements off the lerp chain', diff)
        for x, y, what in zip(a[:3], b[:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert _same(x, y), (route, s, what, 'differs from the run with the average off')
    assert on['updates'] == [1, 2, 3, 4] and off['updates'] == [0, 0, 0, 0]
    assert not _same(on['steps'][3][3], on['steps'][3][0]) and not _same(on['steps'][3][3], on['start'])
    if route == 'clipped':
        assert on['coefs'][0] < 1.0, on['coefs']      # (the bound is half of the first step's norm)
    if route == 'frozen':
        # frozen from the start: identical to its shadow while it rests; then it trains and the shadow follows
        for o, k in on['frozen']:
            assert _same(on['steps'][1][3][o:o + k], on['steps'][1][0][o:o + k]) and _same(on['steps'][1][0][o:o + k], on['p0'][o:o + k])
            assert not _same(on['steps'][3][0][o:o + k], on['p0'][o:o + k])
            assert not _same(on['steps'][3][3][o:o + k], on['steps'][3][0][o:o + k])


# ---------------------------------------------------------------------------------------------------------------------------
# 4, 7, 8. recorded = eager; ema_weights(); off is off
# ---------------------------------------------------------------------------------------------------------------------------
REPLAYS = 5
TOTAL = 2 + REPLAYS                                # one warm-up step, the recording step, the replays


def _outputs(model, batch):
    model.eval()
    with torch.no_grad():
        out = model(dict(batch))
    model.train()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _recorded(ema, swap_after=None, keyword=True):
    """the recorded route: flags, commands per stream, the state after every step from the recording step on; `swap_after`: an
    evaluation under ema_weights() between two replays"""
    from lirec_amd import model as M
    from lirec_amd.graph import RecordedTrainStep
    try:
        model, loss, optim, batch = TC._fresh(side=True)
        if keyword:
            optim.ema_decay = ema
        out = {'steps': [None]}
        g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
        try:
            torch.cuda.synchronize()
            out['flags'] = (g.overwrite, g.fused, g.defer)
            side = model._wgrad_lane()[0].cuda_stream
            cmds = [g.cmds.command(i) for i in range(g.cmds.size)]
            out['launches_side'] = sum(1 for s, k in cmds if k == 0 and s == side)
            out['launches_other'] = sum(1 for s, k in cmds if k == 0 and s != side)
            out['others'] = sum(1 for s, k in cmds if k != 0)
            lanes = {}
            out['commands'] = [(lanes.setdefault(s, len(lanes)), k) for s, k in cmds]
            out['layout'] = (model.lanes.bucket0_end, model.first_layer_range()[0], model.flat_params().numel())

            def snap():
                torch.cuda.synchronize()
                return tuple(t.cpu() for t in TC._state(model, optim)) + (None if optim.ema is None else optim.ema.cpu(),)
            out['steps'].append(snap())
            for r in range(1, REPLAYS + 1):
                g.step()
                out['steps'].append(snap())
                if swap_after == r:
                    before = model.flat_params().clone()
                    with optim.ema_weights():
                        assert _same(model.flat_params(), optim.ema)
                        inside = _outputs(model, batch)
                    assert _same(model.flat_params(), before), 'the training parameters were not restored bit for bit'
                    out['inside'] = inside
                    out['live'] = _outputs(model, batch)
                    sd = {k: v.clone() for k, v in optim.ema_state_dict().items()}
                    fresh, _, _ = M.create_model(101, n_rels=15)
                    fresh.load_state_dict(sd, strict=True)
                    out['fresh'] = _outputs(fresh, batch)
                    del fresh
            out['updates'] = optim.ema_updates()
            out['state'] = g.state.tolist()
            if ema is not None:
                optim.ema_decay = 0.99
                with pytest.raises(RuntimeError, match='hyper-parameters changed'):
                    g.step()
                optim.ema_decay = ema
        finally:
            g.release()
        return out
    finally:
        config.reset()


def test_recorded_is_eager_with_the_average_on():
    """warm-up, recording step and five replays against seven eager steps: shadow, parameters and moments by bits after every
    step from the recording on, the folded first-layer update and the un-joined side stream included; the command list is the one
    with the average off plus exactly the lerps the placement rule predicts, each on its stretch's stream"""
    eager = _cached(('eager', 'side', DECAY, TOTAL), lambda: _eager('side', DECAY, TOTAL))
    rec = _cached(('recorded', DECAY), lambda: _recorded(DECAY))
    base = _cached(('recorded', None), lambda: _recorded(None))
    assert rec['flags'] == base['flags'] == (True, True, True), (rec['flags'], base['flags'])
    assert rec['state'][1:] == [TOTAL, TOTAL] and rec['updates'] == TOTAL
    for s in range(1, TOTAL):
        for x, y, what in zip(eager['steps'][s], rec['steps'][s], ('parameters', 'exp_avg', 'exp_avg_sq', 'shadow')):
            assert _same(x, y), (s + 1, what, int((_bits(x) != _bits(y)).sum()))
    for s in range(1, TOTAL):
        for x, y, what in zip(base['steps'][s][:3], rec['steps'][s][:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
            assert _same(x, y), (s + 1, what, 'the average changed the recorded step')
    # the placement rule: the side stream's bucket [0, hi0) behind its Adam launch on the side stream; on the caller's stream
    # the stretch [hi0, lo) behind its Adam launch and the folded first-layer range [lo, end) from step()
    hi0, lo, end = rec['layout']
    assert 0 < hi0 < lo < end
    assert rec['launches_side'] == base['launches_side'] + 1, (rec['launches_side'], base['launches_side'])
    assert rec['launches_other'] == base['launches_other'] + 2, (rec['launches_other'], base['launches_other'])
    assert rec['others'] == base['others'] and len(rec['commands']) == len(base['commands']) + 3


def test_ema_weights_swaps_by_value_and_a_replay_after_it_is_the_eager_continuation():
    eager = _cached(('eager', 'side', DECAY, TOTAL), lambda: _eager('side', DECAY, TOTAL))
    rec = _cached(('recorded', DECAY, 'swap'), lambda: _recorded(DECAY, swap_after=3))
    for k in rec['inside']:
        assert _same(rec['inside'][k], rec['fresh'][k]), (k, 'inside ema_weights() vs a fresh model loaded with ema_state_dict()')
    assert any(not _same(rec['inside'][k], rec['live'][k]) for k in rec['inside']), 'the averaged weights computed the live outputs'
    for s in range(1, TOTAL):
        for x, y, what in zip(eager['steps'][s], rec['steps'][s], ('parameters', 'exp_avg', 'exp_avg_sq', 'shadow')):
            assert _same(x, y), (s + 1, what, 'a replay after the swap left the eager continuation')


def test_off_is_off():
    """ema_decay=None: no shadow is ever allocated, and the recorded command list is the one recorded without the keyword --
    the same commands on the same streams in the same order"""
    none = _cached(('recorded', None), lambda: _recorded(None))
    plain = _cached(('recorded', 'no keyword'), lambda: _recorded(None, keyword=False))
    assert all(s is None or s[3] is None for s in none['steps'])
    assert none['flags'] == plain['flags'] and none['commands'] == plain['commands'] and none['updates'] == 0
    on = _cached(('recorded', DECAY), lambda: _recorded(DECAY))
    assert len(on['commands']) > len(none['commands'])
    for s in range(1, TOTAL):
        for x, y in zip(none['steps'][s][:3], plain['steps'][s][:3]):
            assert _same(x, y)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a poisoned step under skip_nonfinite
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_is_no_update_of_the_average():
    """five guarded steps, a NaN written into one trainable gradient element between backward and step() of step 3: the shadow
    keeps its bits, ema_updates() does not move, and steps 4 and 5 go on from there -- the chain of four lerps"""
    try:
        model, loss, optim, batch = TC._fresh(side=True)
        optim.skip_nonfinite = True
        optim.ema_decay = DECAY
        w = ops.ema_weight(DECAY)
        name = next(n for n in model._offsets if n.endswith('.weight'))
        at = model._offsets[name][0] + 3
        chain, counts = None, []
        for s in (1, 2, 3, 4, 5):
            TC._backward(model, loss, optim, batch)
            if chain is None:
                chain = optim.ema.cpu()
            if s == 3:
                model.flat_grads(attach=False)[at] = float('nan')
                torch.cuda.synchronize()
            before = optim.ema.clone()
            p_before = model.flat_params().clone()
            optim.step()
            torch.cuda.synchronize()
            counts.append(optim.ema_updates())
            if s == 3:
                assert float(optim.found_nonfinite) == 1.0
                assert _same(optim.ema, before), 'the skipped step moved the shadow'
                assert _same(model.flat_params(), p_before)
            else:
                assert float(optim.found_nonfinite) == 0.0
                chain = torch.lerp(chain, model.flat_params().cpu(), w)
                assert not _same(optim.ema, before)
            assert _same(optim.ema, chain), s
        assert counts == [1, 2, 2, 3, 4] and optim.skipped_total() == 1
        optim.ema_reset()
        torch.cuda.synchronize()
        assert _same(optim.ema, model.flat_params()) and optim.ema_updates() == 0
    finally:
        config.reset()


def test_a_skipped_replay_is_no_update_of_the_average():
    """the same on the recorded route: the recorded lerp launches hold the guard block's ADDRESS, so a replay on a batch with a
    NaN feature leaves the shadow's bits alone and the next replays go on from them"""
    import test_gpu_guard as TG
    from lirec_amd.graph import RecordedTrainStep
    try:
        model, loss, optim, batch = TC._fresh(side=True)
        optim.skip_nonfinite = True
        optim.ema_decay = DECAY
        w = ops.ema_weight(DECAY)
        spot = TG._poison_spot(batch)
        keep = spot.clone()
        g = RecordedTrainStep(model, loss, optim, batch, warmup=1)
        try:
            torch.cuda.synchronize()
            assert optim.ema_updates() == 2
            for s in (3, 4, 5):
                spot.fill_(float('nan')) if s == 4 else spot.copy_(keep)
                before, count = optim.ema.cpu(), optim.ema_updates()
                g.step()
                torch.cuda.synchronize()
                if s == 4:
                    assert float(optim.found_nonfinite) == 1.0
                    assert _same(optim.ema, before) and optim.ema_updates() == count
                else:
                    assert float(optim.found_nonfinite) == 0.0
                    assert _same(optim.ema, torch.lerp(before, model.flat_params().cpu(), w)) and optim.ema_updates() == count + 1
                    assert not _same(optim.ema, before)
            assert optim.ema_updates() == 4 and optim.skipped_total() == 1
        finally:
            g.release()
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_validates_on_the_average_and_checkpoints_it(tmp_path, monkeypatch):
    """opt.ema_decay / opt.eval_ema through create_model and training(): the 'val' evaluation sees the shadow's values, the
    'train' one the live weights, which are back bit for bit afterwards; the final checkpoint carries the average beside an
    optimizer entry that a fresh FusedAdam loads, and load_model(ema=True) / load_ema read it"""
    import os
    from lirec_amd import model as M, train, util
    from lirec_amd.data import SyntheticMixedFeaturesDataset
    dims = dict(text_dim=24, visual_dim=32, track_dim=32)
    try:
        config.recipe('int_rel_ch', joint_dim=16, batch_size=4, num_workers=0, epochs=2, test_fr=1, store_root=str(tmp_path),
                      rels_n_clips=3, ema_decay=0.9, eval_ema=True, **dims)
        opt.device = 'cuda'
        kw = dict(T=6, R=3, n_classes=11, n_rels=5, n_mgd=11, soft_gt=opt.soft_gt, **dims)
        mk = lambda n, seed: SyntheticMixedFeaturesDataset('int_rel_ch', n, seed=seed, **kw)
        model, loss, optim = M.create_model(11, n_rels=5)
        assert optim.ema_decay == 0.9
        seen, real = [], train.testing

        def noting(dataset, mdl, *a, **k):
            torch.cuda.synchronize()
            seen.append((k.get('mode'), mdl.flat_params().clone(), optim.ema.clone()))
            return real(dataset, mdl, *a, **k)
        monkeypatch.setattr(train, 'testing', noting)
        training_set = mk(9, 1)
        train.training(training_set, model=model, loss=loss, optimizer=optim, test_dataset=mk(8, 2))
        torch.cuda.synchronize()
        assert [m for m, _, _ in seen] == ['train', 'val', 'train', 'val']
        for mode, params, shadow in seen:
            assert _same(params, shadow) == (mode == 'val'), mode
        assert not _same(model.flat_params(), optim.ema), 'the live weights were left swapped, or the shadow never moved'
        steps = optim._step
        assert steps > 0 and optim.ema_updates() == steps
        path = os.path.join(str(tmp_path), '1.pth.tar')
        ck = torch.load(path, weights_only=False)
        assert set(ck) == {'epoch', 'state_dict', 'optimizer', 'ema'}
        assert ck['ema']['decay'] == 0.9 and ck['ema']['updates'] == steps
        m2, _, o2 = M.create_model(11, n_rels=5)
        m2.load_state_dict(util.load_model(path=path))
        o2.load_state_dict(util.load_optimizer(path=path))
        assert util.load_ema(o2, path=path)
        torch.cuda.synchronize()
        assert _same(m2.flat_params(), model.flat_params()) and _same(o2.ema, optim.ema) and o2.ema_updates() == steps
        m3, _, _ = M.create_model(11, n_rels=5)
        m3.load_state_dict(util.load_model(path=path, ema=True))
        assert _same(m3.flat_params(), optim.ema)
    finally:
        config.reset()
