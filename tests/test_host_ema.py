"""The weight average (FusedAdam.ema_decay, lirec_ema_step) as far as a host without a GPU can check it: the export and the ABI
number, every refusal of lirec_ema_step (they come before any device call), the validation of the decay, the recorded step's key,
the checkpoint formats, and a dry run of the whole host stack -- eager, guarded and recorded -- with the average on, which also
counts the recorded launches.
"""
import ctypes as C
import importlib.util
import inspect
import math
import os
import subprocess
import sys

import pytest
import torch

from lirec_amd import _lib, config, ops, util
from lirec_amd.config import opt
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = _lib.LIREC_EINVAL
DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)


def test_export_and_abi_number():
    assert 'lirec_ema_step' in _lib.EXPORTS
    L = _lib.lib()
    assert _lib.ABI_VERSION == 124 and L.lirec_version() == 124
    assert L.lirec_ema_step.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    assert _lib.EMA_MAX_BLOCKS == 2048


def _aligned(n_floats):
    raw = (C.c_float * (n_floats + 8))()
    base = C.addressof(raw)
    return raw, base + (-base) % 16


def test_every_refusal_comes_before_a_device_call():
    """no device in this process: a call that got past its checks would try to launch"""
    f = _lib.lib().lirec_ema_step
    keep_e, e = _aligned(64)
    keep_p, p = _aligned(64)
    keep_g, g = _aligned(8)
    ok_w = 0.1
    table = {
        'ema NULL': (None, p, 8, ok_w, None),
        'p NULL': (e, None, 8, ok_w, None),
        'both NULL': (None, None, 8, ok_w, None),
        'n < 0': (e, p, -1, ok_w, None),
        'ema not 4-byte aligned': (e + 2, p + 2, 8, ok_w, None),
        'p not 4-byte aligned': (e, p + 1, 8, ok_w, None),
        'guard not 4-byte aligned': (e, p, 8, ok_w, g + 2),
        'ema and p differ modulo 16 (by 4)': (e, p + 4, 8, ok_w, None),
        'ema and p differ modulo 16 (by 8)': (e + 8, p, 8, ok_w, None),
        'ema and p differ modulo 16 (by 12)': (e + 12, p, 8, ok_w, None),
        'weight 0': (e, p, 8, 0.0, None),
        'weight negative': (e, p, 8, -0.1, None),
        'weight 0.5': (e, p, 8, 0.5, None),
        'weight above 0.5': (e, p, 8, 0.75, None),
        'weight 1': (e, p, 8, 1.0, None),
        'weight NaN': (e, p, 8, float('nan'), None),
        'weight Inf': (e, p, 8, float('inf'), None),
        'n == 0 does not excuse a bad weight': (e, p, 0, 0.5, None),
        'n == 0 does not excuse a NULL': (None, p, 0, ok_w, None),
    }
    for what, (a, b, n, w, gd) in table.items():
        assert f(a, b, n, w, gd, None) == EINVAL, what
    # n == 0 with good arguments: no launch, no error -- at every common offset
    for off in (0, 4, 8, 12):
        assert f(e + off, p + off, 0, ok_w, None, None) == 0
        assert f(e + off, p + off, 0, ok_w, g, None) == 0
    del keep_e, keep_p, keep_g


def test_the_weight_is_the_fp32_rounding_of_the_double_difference():
    for d in (0.9, 0.99, 0.999, 0.9999, 0.51, 0.75):
        w = ops.ema_weight(d)
        assert w == torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32).item()
        assert 0.0 < w < 0.5
    # what torch does with the Python scalar of lerp_: the same float
    e, p = torch.tensor([1.0, -2.0, 3.5]), torch.tensor([0.25, 7.0, 3.5])
    w = ops.ema_weight(0.9)
    want = (torch.tensor(w, dtype=torch.float64) * (p - e).double() + e.double()).float()
    assert torch.equal(torch.lerp(e, p, 1.0 - 0.9), want)


@pytest.mark.parametrize('bad', [0.5, 1.0, -1, float('nan'), 0.0, 0.25, 2.0, float('inf')])
def test_decay_validation_in_the_constructor_and_the_setter(bad):
    try:
        config.recipe('int_rel_ch', joint_dim=16, rels_n_clips=3, **DIMS)
        opt.device = 'cpu'
        from lirec_amd import model as M
        model, _, optim = M.create_model(11, n_rels=5)
        with pytest.raises(ValueError, match='ema_decay'):
            FusedAdam(model, ema_decay=bad)
        with pytest.raises(ValueError, match='ema_decay'):
            optim.ema_decay = bad
        assert optim.ema_decay is None and optim.ema is None
        optim.ema_decay = 0.9
        assert optim.ema_decay == 0.9
        with pytest.raises(ValueError, match='ema_decay'):
            optim.ema_decay = bad
        assert optim.ema_decay == 0.9              # (a refused value leaves the old one)
        optim.ema_decay = None
        assert optim.ema_decay is None
    finally:
        config.reset()


def test_the_keyword_and_the_config_entries():
    assert inspect.signature(FusedAdam.__init__).parameters['ema_decay'].default is None
    assert opt.ema_decay == 0.0 and opt.eval_ema is False
    assert inspect.signature(util.load_model).parameters['ema'].default is False


class _Opt:
    def __init__(self, **kw):
        self.param_groups = [dict(lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)]
        self.grad_scale = 1.0
        self.__dict__.update(kw)


def test_recording_key_carries_the_decay_last_and_only_when_on():
    base = RecordedTrainStep.hyper_key(_Opt())                    # (a stand-in without the attribute: the key as it always was)
    assert base == (3e-5, (0.9, 0.999), 1e-8, 1e-5, 1.0)
    assert RecordedTrainStep.hyper_key(_Opt(ema_decay=None)) == base
    assert RecordedTrainStep.hyper_key(_Opt(ema_decay=0.9)) == base + (('ema_decay', 0.9),)
    assert RecordedTrainStep.hyper_key(_Opt(ema_decay=0.99)) != RecordedTrainStep.hyper_key(_Opt(ema_decay=0.9))
    every = RecordedTrainStep.hyper_key(_Opt(ema_decay=0.9, skip_nonfinite=True, max_grad_norm=2.0))
    assert every == base + (('max_grad_norm', 2.0), ('skip_nonfinite', True), ('ema_decay', 0.9))
    assert RecordedTrainStep.hyper_key(_Opt(ema_decay=None, skip_nonfinite=True)) == base + (('skip_nonfinite', True),)


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------------
def _cpu_pair(**kw):
    config.recipe('int_rel_ch', joint_dim=16, rels_n_clips=3, **DIMS)
    opt.device = 'cpu'
    for k, v in kw.items():
        setattr(opt, k, v)
    from lirec_amd import model as M
    torch.manual_seed(3)
    return M.create_model(11, n_rels=5)


def _tool():
    spec = importlib.util.spec_from_file_location('checkpoint_tool', os.path.join(ROOT, 'tools', 'checkpoint_tool.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_checkpoint_with_the_average_round_trips(tmp_path, monkeypatch):
    try:
        model, _, optim = _cpu_pair(ema_decay=0.9)
        assert optim.ema_decay == 0.9 and optim.ema is None       # (made with the state, not by the constructor)
        optim._ensure_state()
        assert optim.ema is not None and optim.ema.data_ptr() != model.flat_params().data_ptr()
        assert torch.equal(optim.ema, model.flat_params()) and optim.ema_updates() == 0
        # a shadow that is not the parameters, and moments that are not zero
        sd = {k: v + 0.125 for k, v in optim.ema_state_dict().items()}
        optim.load_ema_state_dict(sd, updates=7)
        optim._m.add_(0.5); optim._v.add_(0.25)
        gaps = torch.ones(optim.ema.numel(), dtype=torch.bool)
        for off, k in model._offsets.values():
            gaps[off:off + k] = False
        assert bool((optim.ema[gaps] == 0).all()), 'the alignment gaps of the shadow are zeros'
        path = str(tmp_path / 'ck.pth.tar')
        util.save_checkpoint(path, 3, model, optim)
        ck = torch.load(path, map_location='cpu', weights_only=False)
        assert sorted(ck) == ['ema', 'epoch', 'optimizer', 'state_dict']
        assert ck['ema']['decay'] == 0.9 and ck['ema']['updates'] == 7
        assert list(ck['ema']['state_dict']) == list(ck['state_dict'])
        for k, v in ck['state_dict'].items():
            assert torch.equal(ck['ema']['state_dict'][k], v + 0.125), k
        # the optimizer entry is still what a stock Adam takes, and gives back
        assert sorted(ck['optimizer']) == ['param_groups', 'state']
        stock = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in model.parameters()], lr=opt.lr, weight_decay=opt.weight_decay)
        stock.load_state_dict(ck['optimizer'])
        back = stock.state_dict()
        for i, p in enumerate(model.parameters()):
            assert torch.equal(back['state'][i]['exp_avg'], torch.full_like(p, 0.5)), i
            assert torch.equal(back['state'][i]['exp_avg_sq'], torch.full_like(p, 0.25)), i
        # load_model(ema=True), and back into a fresh optimiser
        got = util.load_model(path=path, ema=True)
        assert all(torch.equal(got[k], sd[k]) for k in sd)
        assert all(torch.equal(util.load_model(path=path)[k], v) for k, v in model.state_dict().items())
        model2, _, optim2 = _cpu_pair(ema_decay=0.9)
        model2.load_state_dict(util.load_model(path=path))
        optim2.load_state_dict(util.load_optimizer(path=path))
        assert util.load_ema(optim2, path=path) is True
        assert torch.equal(optim2.ema, optim.ema) and optim2.ema_updates() == 7
        # the tool writes the averaged weights as a plain checkpoint
        out = str(tmp_path / 'ema_only.pth.tar')
        monkeypatch.setattr(sys, 'argv', ['checkpoint_tool.py', 'ema', path, out])
        _tool().main()
        plain = torch.load(out, map_location='cpu', weights_only=False)
        assert sorted(plain) == ['epoch', 'state_dict'] and plain['epoch'] == 3
        model3, _, _ = _cpu_pair()
        model3.load_state_dict(plain['state_dict'], strict=True)
        assert torch.equal(model3.flat_params(), optim.ema)
    finally:
        config.reset()


def test_a_checkpoint_without_the_average_loads_and_the_shadow_starts_from_the_parameters(tmp_path):
    try:
        model, _, optim = _cpu_pair()
        assert optim.ema_decay is None
        optim._ensure_state()
        assert optim.ema is None
        path = str(tmp_path / 'ck.pth.tar')
        util.save_checkpoint(path, 1, model, optim)
        ck = torch.load(path, map_location='cpu', weights_only=False)
        assert sorted(ck) == ['epoch', 'optimizer', 'state_dict']
        with pytest.raises(KeyError, match='EMA'):
            util.load_model(path=path, ema=True)
        model2, _, optim2 = _cpu_pair(ema_decay=0.99)
        with torch.no_grad():
            for p in model2.parameters():
                p.add_(1.0)                              # (not the checkpoint's values)
        model2.load_state_dict(util.load_model(path=path))
        optim2.load_state_dict(util.load_optimizer(path=path))
        assert util.load_ema(optim2, path=path) is False
        optim2._ensure_state()
        assert torch.equal(optim2.ema, model.flat_params()) and optim2.ema_updates() == 0
    finally:
        config.reset()


def test_the_shadow_is_kept_when_the_average_is_switched_off_and_reset_copies():
    try:
        model, _, optim = _cpu_pair(ema_decay=0.9)
        optim._ensure_state()
        optim.load_ema_state_dict({k: v + 1.0 for k, v in optim.ema_state_dict().items()}, updates=4)
        kept = optim.ema.clone()
        optim.ema_decay = None
        assert optim.ema is not None and torch.equal(optim.ema, kept) and optim.ema_updates() == 4
        assert RecordedTrainStep.hyper_key(optim) == RecordedTrainStep.hyper_key(_cpu_pair()[2])
        optim.ema_decay = 0.99
        assert torch.equal(optim.ema, kept) and optim.ema_updates() == 4
        optim.ema_reset()
        assert torch.equal(optim.ema, model.flat_params()) and optim.ema_updates() == 0
        # a state_dict of the optimiser has no trace of the average
        assert sorted(optim.state_dict()) == ['param_groups', 'state']
        assert 'ema_decay' not in optim.state_dict()['param_groups'][0]
    finally:
        config.reset()


# ---------------------------------------------------------------------------------------------------------------------------
# the host stack with the average on, launches handed to nobody (host_dryrun): eager, guarded, recorded, replayed
# ---------------------------------------------------------------------------------------------------------------------------
def test_dry_run_of_the_host_stack_with_the_average_on():
    """... and the recorded launches counted: no side streams in a dry run and nothing folded at the small shape, so the whole
    buffer is ONE stretch on the caller's stream: one lerp more than with the average off, guarded or not"""
    code = ('import host_dryrun as H, torch\n'
            'from lirec_amd import _lib, ops, config\n'
            'from lirec_amd.config import opt\n'
            'from lirec_amd.graph import RecordedTrainStep\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'small = dict(text_dim=24, visual_dim=32, track_dim=32, joint_dim=16)\n'
            'big = dict(text_dim=768, visual_dim=2048, track_dim=2048, joint_dim=512)\n'
            'ops.set_gemm_mode(2)\n'
            'sizes = {}\n'
            'real = RecordedTrainStep.__init__\n'
            'def noting(self, *a, **k):\n'
            '    real(self, *a, **k)\n'
            '    sizes[(self.optim.ema_decay, bool(self.optim.skip_nonfinite))] = (self.cmds.size, self.fused)\n'
            'RecordedTrainStep.__init__ = noting\n'
            'for kind, a in (("int_rel_ch", (11, 5, 4, 6, 3)), ("int_rels", (11, 5, 5, 1, 3)), ("int_ch", (11, 5, 4, 6, 0))):\n'
            '    sizes.clear()\n'
            '    for ema in (0.0, 0.9):\n'
            '        for guard in (False, True):\n'
            '            H.one_recipe(kind, small, *a, ema_decay=ema, skip_nonfinite=guard)\n'
            '    assert not any(f for _, f in sizes.values()), sizes\n'
            '    for guard in (False, True):\n'
            '        assert sizes[(0.9, guard)][0] == sizes[(None, guard)][0] + 1, (kind, sizes)\n'
            'm = H.one_recipe("int_rel_ch", big, 101, 15, 8, 16, 18, steps=1, features="q32", ema_decay=0.99)\n'
            'opt.ema_decay = 0.0; opt.skip_nonfinite = False\n'
            'print("ema dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'ema dry run ok' in r.stdout, r.stdout[-4000:]


def test_swaps_and_resets_are_refused_inside_a_recording():
    try:
        model, _, optim = _cpu_pair(ema_decay=0.9)
        optim._ensure_state()
        ops.CommandList.begin()
        try:
            assert ops.CommandList.mark() >= 0
            with pytest.raises(RuntimeError, match='recorded'):
                with optim.ema_weights():
                    pass
            with pytest.raises(RuntimeError, match='recorded'):
                optim.ema_reset()
            with pytest.raises(RuntimeError, match='recorded'):
                optim.load_ema_state_dict(optim.ema_state_dict())
        finally:
            ops.CommandList.end().destroy()
        # outside: parameters <-> shadow by value, restored bit for bit, the buffers' addresses unchanged
        optim.load_ema_state_dict({k: v * 2 + 1 for k, v in optim.ema_state_dict().items()})
        flat = model.flat_params()
        before, addr = flat.clone(), flat.data_ptr()
        model._w1q_valid, model.lanes.bucket0_on_side = True, True
        with optim.ema_weights():
            assert torch.equal(flat, optim.ema) and not torch.equal(flat, before)
            assert model._w1q_valid is False and model.lanes.bucket0_on_side is False
            model._w1q_valid, model.lanes.bucket0_on_side = True, True
        assert torch.equal(flat.view(torch.int32), before.view(torch.int32)) and model.flat_params().data_ptr() == addr
        assert model._w1q_valid is False and model.lanes.bucket0_on_side is False
        assert math.isfinite(float(flat.sum()))
    finally:
        config.reset()
