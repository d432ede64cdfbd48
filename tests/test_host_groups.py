"""Parameter groups and device-resident hyper-parameters without a GPU: the yardstick of the GPU tests against torch.optim.Adam in
float64; the fp32 restatement inside adam_cases' bounds on every case tests/test_gpu_groups.py runs; the grouped ranges against a
per-element brute force; the argument checks of lirec_adam_hyper_write, lirec_adam_step_groups and lirec_set_adam_hyper_row
through the C ABI (LIREC_EINVAL before any device call), with and without the library's host-side dry run; the whole host stack
with three groups in the dry run; checkpoints to a stock torch.optim.Adam with the same groups and back; the constructor's
refusals; the recorded step's key."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_cases as AC
import group_cases as GC
from lirec_amd import _lib, config, util
from lirec_amd.config import opt
from lirec_amd.graph import RecordedTrainStep
from lirec_amd.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = 4194304                                  # lirec_debug_set: host-side dry run (tests/host_dryrun.py)
EINVAL = _lib.LIREC_EINVAL


def _model(kind='int_rel_ch'):
    from lirec_amd import model as M
    config.recipe(kind, joint_dim=GC.JOINT, rels_n_clips=GC.R, dropout=0.3, dropout_seed=7, **GC.DIMS)
    opt.device = 'cpu'
    torch.manual_seed(3)
    return M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)


def _grouped(model, **kw):
    return FusedAdam(model, lr=3e-5, weight_decay=1e-5, param_groups=GC.three_groups(model), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick is torch
# ---------------------------------------------------------------------------------------------------------------------------
def test_ref64_per_group_is_torch_adam_in_float64():
    """six parameters in three groups (the rows of the kernel cases), three steps, parameter 3 frozen for the second: ref64 range
    by range -- the frozen parameter left out of step 2 and one step behind in step 3 -- against torch.optim.Adam on float64 CPU
    tensors with the same groups, fed g * grad_scale (a power of two: exact), to 1e-12 relative"""
    sizes, group_of = [5, 7, 16, 3, 9, 4], [0, 1, 2, 0, 1, 2]
    rows = [AC.hyper32(r + (1.0,))[:5] for r in GC.ROWS]
    r = np.random.default_rng(5)
    offs, at = [], 0
    for k in sizes:
        offs.append(at)
        at = (at + k + 3) // 4 * 4
    p = np.zeros(at, np.float32)
    for o, k in zip(offs, sizes):
        p[o:o + k] = (0.1 * r.standard_normal(k)).astype(np.float32)
    params = [torch.nn.Parameter(torch.from_numpy(p[o:o + k].astype(np.float64))) for o, k in zip(offs, sizes)]
    ref = torch.optim.Adam([dict(params=[q for q, g in zip(params, group_of) if g == i], lr=rows[i][0], betas=rows[i][1:3],
                                 eps=rows[i][3], weight_decay=rows[i][4]) for i in range(3)])
    P, M, V = p.astype(np.float64), np.zeros(at), np.zeros(at)
    lag = [0] * len(sizes)
    worst = 0.0
    for step in (1, 2, 3):
        g = np.zeros(at, np.float32)
        for o, k in zip(offs, sizes):
            g[o:o + k] = r.standard_normal(k).astype(np.float32)
        frozen = {3} if step == 2 else set()
        for i, (q, o, k) in enumerate(zip(params, offs, sizes)):
            q.grad = None if i in frozen else torch.from_numpy(g[o:o + k].astype(np.float64) * GC.GRAD_SCALE)
        ref.step()
        rs = [(o, k, lag[i], group_of[i]) for i, (o, k) in enumerate(zip(offs, sizes)) if i not in frozen]
        P, M, V = GC.ref64(P, g, M, V, rs, step, rows, GC.GRAD_SCALE)[:3]
        for i in frozen:
            lag[i] += 1
        for i, (q, o, k) in enumerate(zip(params, offs, sizes)):
            st = ref.state[q]
            assert int(st['step']) == step - lag[i]
            for got, want in ((P[o:o + k], q.detach().numpy()), (M[o:o + k], st['exp_avg'].numpy()), (V[o:o + k], st['exp_avg_sq'].numpy())):
                err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
                worst = max(worst, float(err.max()))
                assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (step, i, float(err.max()))
    print('ref64 per group against torch.optim.Adam (float64): worst relative difference %.3g' % worst)
    assert lag[3] == 1


@pytest.mark.parametrize('coef', [1.0, GC.COEF])
@pytest.mark.parametrize('rows', ['ROWS', 'ROWS_B'])
@pytest.mark.parametrize('step', GC.STEPS)
def test_fp32_restatement_per_group_stays_inside_the_bounds(step, rows, coef):
    """every case of tests/test_gpu_groups.py's kernel tests (three steps, both tables of rows, unclipped and clipped): ref32 range
    by range uses less than 1.0 of every adam_cases bound -- the GPU tests may hold the kernels to those bounds unchanged"""
    rows = getattr(GC, rows)
    s, rs = GC.build(step)
    got = GC.ref32(*s, rs, step, rows, GC.GRAD_SCALE, coef)
    use = GC.use_of_bounds(got, *s, rs, step, rows, GC.GRAD_SCALE, coef)
    print('step %d coef %g: use of the bounds p %.3f m %.3f v %.3f' % (step, coef, *use))
    assert max(use) < 1.0, use
    mask = GC.inside(rs, len(s[0]))
    for a, b in zip(got, (s[0], s[2], s[3])):
        assert np.array_equal(a[~mask], b[~mask])


def test_the_kernel_cases_are_what_the_issue_asks_for():
    rs, n = GC.ranges()
    assert [k for _, k, _, _ in rs] == [1, 3, 4, 5, 1023, 1024, 1025, 4099]
    assert {g for _, _, _, g in rs} == {0, 1, 2} and {lag for _, _, lag, _ in rs} == {0, 2}
    assert all(o % 4 == 0 for o, _, _, _ in rs)
    assert all(b[0] - (a[0] + a[1]) >= GC.GUARD for a, b in zip(rs, rs[1:])) and rs[0][0] >= GC.GUARD and n - (rs[-1][0] + rs[-1][1]) >= GC.GUARD
    assert GC.ROWS == [tuple(h[:5]) for h in AC.HYPERS[:3]]
    # ... and they are ranges FusedAdam's own merge leaves as they are (no two touch): one parameter each
    offsets = {'r%d' % i: (o, k) for i, (o, k, _, _) in enumerate(rs)}
    merged = FusedAdam.merged_ranges(offsets, {n: True for n in offsets}, {'r%d' % i: lag for i, (_, _, lag, _) in enumerate(rs)},
                                     rs[-1][0] + rs[-1][1], {'r%d' % i: g for i, (_, _, _, g) in enumerate(rs)})
    assert merged == [(o, o + k, lag, g) for o, k, lag, g in rs]


# ---------------------------------------------------------------------------------------------------------------------------
# grouped ranges
# ---------------------------------------------------------------------------------------------------------------------------
def _brute(offsets, trainable, lags, groups, extent):
    """per element: (lag, group) of the trainable parameter it belongs to, or None"""
    owner = [None] * extent
    for n, (o, k) in offsets.items():
        if trainable[n]:
            for i in range(o, o + k):
                owner[i] = (int(lags.get(n, 0)), int(groups[n]))
    return owner


def _parent_merged_ranges(offsets, trainable, lags, extent):
    """FusedAdam.merged_ranges as it was before parameter groups, word for word"""
    out, prev_live = [], False
    names = list(offsets)
    for i, n in enumerate(names):
        off, k = offsets[n]
        live = bool(trainable[n])
        if live:
            end = extent if i == len(names) - 1 else off + k
            lag = int(lags.get(n, 0))
            if prev_live and out[-1][2] == lag:
                out[-1] = (out[-1][0], end, lag)
            else:
                out.append((off, end, lag))
        prev_live = live
    return out


def test_grouped_merged_ranges_against_a_per_element_brute_force():
    r = np.random.default_rng(17)
    for trial in range(200):
        n_par = int(r.integers(1, 30))
        offsets, at = {}, 0
        for i in range(n_par):
            k = int(r.integers(1, 40))
            offsets['p%d' % i] = (at, k)
            at = (at + k + 3) // 4 * 4 + 4 * int(r.integers(0, 2))
        extent = at + 4 * int(r.integers(0, 3))
        names = list(offsets)
        trainable = {n: bool(r.random() < r.choice([0.3, 0.7, 1.0])) for n in names}
        lags = {n: int(r.integers(0, 3)) for n in names if r.random() < 0.3}
        n_groups = int(r.integers(1, 9))
        groups = {n: int(r.integers(0, n_groups)) for n in names}
        rs = FusedAdam.merged_ranges(offsets, trainable, lags, extent, groups)
        owner = _brute(offsets, trainable, lags, groups, extent)
        covered = [None] * extent
        end = 0
        for a, b, lag, grp in rs:
            assert 0 <= a < b <= extent and a % 4 == 0 and a >= end
            end = b
            for i in range(a, b):
                assert covered[i] is None, 'an element is covered twice'
                covered[i] = (lag, grp)
        in_param = [False] * extent
        for n, (o, k) in offsets.items():
            for i in range(o, o + k):
                in_param[i] = True
        for i in range(extent):
            if owner[i] is not None:
                assert covered[i] == owner[i], (trial, i, 'a trainable element with another lag / group, or not covered')
            elif in_param[i]:
                assert covered[i] is None, (trial, i, 'a frozen element is covered')
        # a covered gap element lies between two trainable neighbours of the layout with the range's lag and group -- or behind the
        # last parameter, when that one is trainable (the buffer's tail)
        for a, b, lag, grp in rs:
            inside = [n for n in names if offsets[n][0] >= a and offsets[n][0] + offsets[n][1] <= b]
            assert inside and all(trainable[n] and lags.get(n, 0) == lag and groups[n] == grp for n in inside)
            idx = [names.index(n) for n in inside]
            assert idx == list(range(idx[0], idx[0] + len(idx))), 'a range skips a parameter of the layout'
        # one group: what it was before groups, as 3-tuples without the keyword and with a constant group appended with it
        parent = _parent_merged_ranges(offsets, trainable, lags, extent)
        assert FusedAdam.merged_ranges(offsets, trainable, lags, extent) == parent
        assert FusedAdam.merged_ranges(offsets, trainable, lags, extent, {n: 0 for n in names}) == [x + (0,) for x in parent]


def test_trainable_ranges_of_the_three_groups():
    model, _, _ = _model()
    fo = _grouped(model)
    assert fo.device_hyper and len(fo.param_groups) == 3
    rs = fo.trainable_ranges()
    mem = dict(zip(fo._names, fo.group_membership()))
    assert rs[0][0] == 0 and rs[-1][1] == model.flat_params().numel()
    for a, b, lag, grp in rs:
        inside = [n for n, (o, k) in model._offsets.items() if o >= a and o + k <= b]
        assert inside and all(mem[n] == grp for n in inside) and lag == 0
    # a stretch is the intersection; 64 ranges a call
    lo, hi = 1056, 12288
    assert fo.trainable_ranges(lo, hi) == [(max(a, lo), min(b, hi), lag, grp) for a, b, lag, grp in rs if min(b, hi) > max(a, lo)]
    # one group, by value: the parent's 3-tuples; one group with device_hyper: the same range with group 0
    plain = FusedAdam(model)
    assert not plain.device_hyper and plain.trainable_ranges() == [(0, model.flat_params().numel(), 0)]
    one = FusedAdam(model, device_hyper=True)
    assert one.device_hyper and one.trainable_ranges() == [(0, model.flat_params().numel(), 0, 0)]
    # freezing alternate parameters of the flat layout: 19 ranges; every one keeps its own group
    pd = dict(model.named_parameters())
    for i, n in enumerate(model._offsets):
        pd[n].requires_grad_(i % 2 == 0)
    rs = fo.trainable_ranges()
    assert len(rs) == 19 and [grp for _, _, _, grp in rs] == [mem[n] for i, n in enumerate(model._offsets) if i % 2 == 0]


# ---------------------------------------------------------------------------------------------------------------------------
# refusals through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
A0 = 0x10000000


def _addr(i):
    return A0 + 0x4000000 * i


TABLE = _addr(8)


@pytest.fixture(params=['dry', 'no_dry_run'])
def lib(request):
    L = _lib.lib()
    if request.param == 'dry':
        assert L.lirec_debug_set(DRY, -1) == 0
    try:
        yield L, request.param == 'dry'
    finally:
        assert L.lirec_set_adam_hyper_row(None) == 0
        assert L.lirec_debug_set(0, -1) == 0


def _rows(n=3):
    arr = (_lib.AdamHyper * max(n, 1))()
    for a, r in zip(arr, (GC.ROWS * 3)[:n]):
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = r
    return arr


def _groups(L, rs=((0, 1023, 0, 0), (1024, 5, 2, 2)), **kw):
    v = dict(p=_addr(0), g=_addr(1), m=_addr(2), v=_addr(3), table=TABLE, n_groups=3, step=3, step_dev=None, count=None, ticket=None,
             advance=0, n=None)
    v.update(kw)
    arr = (_lib.AdamGroupRange * max(len(rs), 1))()
    for a, (o, k, lag, grp) in zip(arr, rs):
        a.offset, a.length, a.lag, a.group = o, k, lag, grp
    n = len(rs) if v['n'] is None else v['n']
    return L.lirec_adam_step_groups(v['p'], v['g'], v['m'], v['v'], arr if v.get('ranges', 1) else None, n, v['table'], v['n_groups'],
                                    v['step'], 1.0, v['step_dev'], v['count'], v['ticket'], v['advance'], None)


def test_abi_of_the_new_calls():
    L = _lib.lib()
    assert L.lirec_version() == _lib.ABI_VERSION == 124
    assert L.lirec_abi_sizeof(11) == C.sizeof(_lib.AdamHyper) == 32
    assert L.lirec_abi_sizeof(12) == C.sizeof(_lib.AdamGroupRange) == 24
    assert L.lirec_abi_sizeof(10) == C.sizeof(_lib.AdamRange) == 24                # (lirec_adam_range is left alone)
    for name in ('lirec_adam_hyper_write', 'lirec_adam_step_groups', 'lirec_set_adam_hyper_row'):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ADAM_MAX_GROUPS == FusedAdam.MAX_GROUPS == 8


BAD_GROUPS = {
    # everything lirec_adam_step_ranges refuses
    'count_negative': dict(n=-1),
    'count_65': dict(rs=tuple((16 * i, 8, 0, 0) for i in range(65))),
    'ranges_null': dict(ranges=0),
    'negative_length': dict(rs=((0, -1, 0, 0),)),
    'negative_length_second': dict(rs=((0, 8, 0, 0), (16, -4, 0, 1))),
    'offset_not_multiple_of_4': dict(rs=((0, 8, 0, 0), (17, 4, 0, 0))),
    'offset_2': dict(rs=((2, 8, 0, 0),)),
    'negative_offset': dict(rs=((-4, 8, 0, 0),)),
    'overlap': dict(rs=((0, 10, 0, 0), (8, 4, 0, 1))),
    'out_of_order': dict(rs=((64, 8, 0, 0), (0, 8, 0, 0))),
    'step_minus_lag_0': dict(rs=((0, 8, 3, 0),)),
    'step_minus_lag_negative': dict(rs=((0, 8, 0, 0), (8, 8, 5, 0))),
    'negative_lag': dict(rs=((0, 8, -1, 0),)),
    'step_0_by_value': dict(step=0),
    'p_null': dict(p=None), 'g_null': dict(g=None), 'm_null': dict(m=None), 'v_null': dict(v=None),
    'both_device_steps': dict(step_dev=_addr(6), count=_addr(4), ticket=_addr(5)),
    'count_without_ticket': dict(count=_addr(4)),
    # the groups' own
    'group_negative': dict(rs=((0, 8, 0, -1),)),
    'group_equal_to_n_groups': dict(rs=((0, 8, 0, 0), (8, 8, 0, 3))),
    'group_7_of_3': dict(rs=((0, 8, 0, 7),)),
    'group_1_of_1': dict(rs=((0, 8, 0, 1),), n_groups=1),
    'n_groups_0': dict(n_groups=0, rs=((0, 8, 0, 0),)),
    'n_groups_negative': dict(n_groups=-1, rs=((0, 8, 0, 0),)),
    'n_groups_9': dict(n_groups=9),
    'table_null': dict(table=None),
    'table_plus4': dict(table=TABLE + 4), 'table_plus8': dict(table=TABLE + 8), 'table_plus12': dict(table=TABLE + 12),
}
BAD_GROUPS.update({'%s_plus%d' % (k, off): {k: _addr(i) + off} for i, k in enumerate('pgmv') for off in (4, 8, 12)})


@pytest.mark.parametrize('what', sorted(BAD_GROUPS))
def test_adam_step_groups_argument_checks(lib, what):
    L, dry = lib
    assert _groups(L, **BAD_GROUPS[what]) == EINVAL
    if what.split('_plus')[0] in ('p', 'g', 'm', 'v', 'table') or what in ('table_null', 'n_groups_9'):
        assert _groups(L, rs=(), **BAD_GROUPS[what]) == EINVAL          # (checked before the count = 0 shortcut)
    # count 0 and all lengths 0: no launch -- also without the dry run
    assert _groups(L, rs=()) == 0
    assert _groups(L, rs=((0, 0, 0, 0), (8, 0, 1, 2))) == 0
    if dry:                                                              # the valid neighbours pass
        assert _groups(L) == 0
        assert _groups(L, rs=tuple((16 * i, 13, i % 3, i % 8) for i in range(64)), n_groups=8, step=3) == 0
        assert _groups(L, rs=((0, 8, 0, 0), (8, 0, 0, 1), (8, 8, 1, 2))) == 0           # touching ranges, an empty one
        assert _groups(L, rs=((0, 8, 7, 0),), step=0, step_dev=_addr(6)) == 0           # (the step is read on the device)
        assert _groups(L, rs=((0, 8, 7, 2),), step=0, count=_addr(4), ticket=_addr(5), advance=1) == 0
        assert _groups(L, p=_addr(0) + 16, g=_addr(1) + 48, m=_addr(2) + 16, v=_addr(3) + 32, table=TABLE + 16) == 0
        assert _groups(L, rs=((0, 8, 0, 0),), n_groups=1) == 0


def test_adam_hyper_write_argument_checks(lib):
    L, dry = lib
    for bad in ((None, _rows(), 3), (TABLE + 4, _rows(), 3), (TABLE + 8, _rows(), 3), (TABLE + 12, _rows(), 3),      # NULL / misaligned table
                (TABLE, _rows(), 0), (TABLE, _rows(), -1), (TABLE, _rows(9), 9),                                      # n_groups outside 1..8
                (TABLE, None, 3)):                                                                                    # no rows
        assert L.lirec_adam_hyper_write(*bad, None) == EINVAL, bad
    if dry:
        for n in (1, 3, 8):
            assert L.lirec_adam_hyper_write(TABLE, _rows(n), n, None) == 0
        assert L.lirec_adam_hyper_write(TABLE + 16, _rows(), 3, None) == 0
        # the values are not the library's to check (a negative learning rate is Python's ValueError)
        rows = _rows(1)
        rows[0].lr, rows[0].beta1 = -1.0, 2.0
        assert L.lirec_adam_hyper_write(TABLE, rows, 1, None) == 0


def test_set_adam_hyper_row_argument_checks(lib):
    L, dry = lib
    for off in (4, 8, 12, 2):
        assert L.lirec_set_adam_hyper_row(TABLE + off) == EINVAL
    assert L.lirec_set_adam_hyper_row(TABLE) == 0 and L.lirec_set_adam_hyper_row(TABLE + 32) == 0
    assert L.lirec_set_adam_hyper_row(None) == 0


def test_the_new_launches_are_recorded_one_command_each():
    L = _lib.lib()
    assert L.lirec_debug_set(DRY, -1) == 0
    try:
        assert L.lirec_record_begin() == 0
        assert L.lirec_adam_hyper_write(TABLE, _rows(), 3, None) == 0
        assert _groups(L) == 0
        assert L.lirec_set_adam_clip(_addr(9)) == 0
        assert _groups(L) == 0                                       # (the clipped kernel)
        assert L.lirec_set_adam_clip(None) == 0
        assert _groups(L, rs=()) == 0                                # nothing
        h = C.c_void_p()
        assert L.lirec_record_end(C.byref(h)) == 0
        kinds = []
        for i in range(L.lirec_cmdlist_size(h)):
            s, k = C.c_void_p(), C.c_int32()
            assert L.lirec_cmdlist_command(h, i, C.byref(s), C.byref(k)) == 0
            kinds.append(k.value)
        assert kinds.count(0) == 3
        assert L.lirec_cmdlist_replay(h, 0, -1) == 0 and L.lirec_cmdlist_destroy(h) == 0
    finally:
        assert L.lirec_set_adam_clip(None) == 0
        assert L.lirec_debug_set(0, -1) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the whole host stack, three groups, in the dry run
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_whole_host_stack_with_three_groups_in_the_dry_run():
    """eager steps, a recording, replays with the learning rates changed in between (no raise, the same command list, one write per
    table and change), a lagged replay, release / resume -- through the real Python host stack (a process of its own: the dry run
    patches torch and switches the library process-wide)"""
    code = ('import host_dryrun as H, torch, group_cases as GC\n'
            'from lirec_amd import _lib, ops, config, model as M\n'
            'from lirec_amd.config import opt\n'
            'from lirec_amd.optim import FusedAdam\n'
            'from lirec_amd.graph import RecordedTrainStep\n'
            'from lirec_amd.data import synthetic_batch\n'
            'L = _lib.lib(); assert L.lirec_debug_set(H.DRY, -1) == 0; H.patch()\n'
            'ops.set_gemm_mode(2)\n'
            'config.recipe("int_rel_ch", dropout=0.3, dropout_seed=5, joint_dim=GC.JOINT, rels_n_clips=GC.R, **GC.DIMS)\n'
            'opt.device = "cpu"; opt.wgrad_side_stream = False\n'
            'model, loss, _ = M.create_model(GC.N_CLASSES, n_rels=GC.N_RELS)\n'
            'optim = FusedAdam(model, lr=3e-5, weight_decay=1e-5, param_groups=GC.three_groups(model))\n'
            'model.train()\n'
            'hb = synthetic_batch(3, "int_rel_ch", GC.B, n_classes=GC.N_CLASSES, n_rels=GC.N_RELS, T=GC.T, R=GC.R, **GC.DIMS)\n'
            'batch = {k: (v.float() if (torch.is_tensor(v) and k == "features") else v) for k, v in hb.items()}\n'
            'writes = []\n'
            'w0 = ops.adam_hyper_write\n'
            'ops.adam_hyper_write = lambda t, rows: (writes.append(rows), w0(t, rows))[1]\n'
            'for _ in range(2):\n'
            '    optim.zero_grad(); lv = loss(model(dict(batch)), batch); lv.backward(); optim.step()\n'
            'assert len(writes) == 1, writes\n'
            'g = RecordedTrainStep(model, loss, optim, batch, warmup=1)\n'
            'n = g.cmds.size\n'
            'assert n > 5 and len(writes) == 1\n'
            'key = g._hyper\n'
            'assert key[0][0] == "device_hyper" and key[0][1] == optim.group_membership()\n'
            'for i in range(3):\n'
            '    for grp in optim.param_groups: grp["lr"] = grp["lr"] * 0.5\n'
            '    g.step()\n'
            '    assert g.cmds.size == n and len(writes) == 2 + i, (i, len(writes))\n'
            'g.step(); assert len(writes) == 4\n'
            'optim.param_groups[2]["weight_decay"] = 1e-3\n'
            'g.lag(n // 2, 10); g.step(); g.lag(None)\n'
            'assert len(writes) == 5 and writes[-1][2][4] == 1e-3\n'
            'g.release()\n'
            'optim.zero_grad(); lv = loss(model(dict(batch)), batch); lv.backward(); optim.step()\n'
            'g.resume(); g.step(); assert g.cmds.size == n and g.hyper_key(optim) == key\n'
            'optim.device_hyper = False\n'
            'try:\n'
            '    g.step(); raise SystemExit("switching device_hyper did not raise")\n'
            'except RuntimeError as e:\n'
            '    assert "hyper-parameters changed" in str(e)\n'
            'optim.device_hyper = True\n'
            'optim.param_groups[0]["lr"] = -1.0\n'
            'try:\n'
            '    g.step(); raise SystemExit("a negative learning rate did not raise")\n'
            'except ValueError as e:\n'
            '    assert "Invalid learning rate" in str(e)\n'
            'g.release(); g.cmds.destroy()\n'
            'print("grouped dry run ok")\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and 'grouped dry run ok' in r.stdout, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------------
def _stock(model, fo):
    """a stock torch.optim.Adam over clones of the parameters, with the groups of `fo`"""
    clone = {id(p): torch.nn.Parameter(p.detach().clone()) for p in model.parameters()}
    groups = [dict({k: v for k, v in g.items() if k in ('lr', 'betas', 'eps', 'weight_decay')}, params=[clone[id(p)] for p in g['params']])
              for g in fo.param_groups]
    return torch.optim.Adam(groups), clone


def _fill_state(model, fo):
    """moments and steps as after a few updates, one parameter two behind (the update itself needs the GPU)"""
    fo._ensure_state()
    torch.manual_seed(11)
    live = torch.zeros(fo._m.numel(), dtype=torch.bool)
    for o, k in model._offsets.values():
        live[o:o + k] = True
    fo._m.copy_(torch.randn_like(fo._m) * live)          # (the alignment gaps hold zeros)
    fo._v.copy_(torch.rand_like(fo._v) * live)
    fo._step = 7
    fo._lag = {'vis2_ctx.weight': 2}


def test_three_groups_to_a_stock_adam_and_back():
    model, _, _ = _model()
    fo = _grouped(model)
    _fill_state(model, fo)
    fo.param_groups[1]['lr'] = 1.25e-4                     # (a schedule has moved it)
    sd = fo.state_dict()
    assert len(sd['param_groups']) == 3 and sorted(i for g in sd['param_groups'] for i in g['params']) == list(range(38))
    assert [len(g['params']) for g in sd['param_groups']] == [len(x) for x in fo.group_names()]
    ref, clone = _stock(model, fo)
    ref.load_state_dict(sd)
    for g, h in zip(ref.param_groups, fo.param_groups):
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad'):
            assert g[k] == h[k], k
        for q, p in zip(g['params'], h['params']):
            assert q is clone[id(p)]
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(ref.state[q][k], fo.state[p][k])
            assert float(ref.state[q]['step']) == float(fo.state[p]['step'])
    # ... and back, into a fresh optimiser with the same groups but the constructor's values
    model2, _, _ = _model()
    fo2 = _grouped(model2)
    assert fo2.param_groups[1]['lr'] == 3e-4
    fo2.load_state_dict(ref.state_dict())
    assert fo2.param_groups[1]['lr'] == 1.25e-4 and fo2.param_groups[2]['betas'] == (0.8, 0.99) and fo2.param_groups[0]['weight_decay'] == 0.0
    assert fo2._step == 7 and fo2._lag == {'vis2_ctx.weight': 2}
    assert torch.equal(fo2._m, fo._m) and torch.equal(fo2._v, fo._v)
    assert fo2.hyper_rows() == fo.hyper_rows()
    # a stock optimiser with OTHER groups is refused as torch refuses it
    with pytest.raises(ValueError):
        FusedAdam(model2).load_state_dict(ref.state_dict())


def test_flat_checkpoints_keep_the_groups():
    model, _, _ = _model()
    fo = _grouped(model)
    _fill_state(model, fo)
    ck = {'epoch': 3, 'state_dict': model.state_dict(), 'optimizer': fo.state_dict(), 'param_group_names': fo.group_names()}
    flat = util.checkpoint_to_flat(ck, model)
    assert flat['step'] == 7 and flat['lags'] == {'vis2_ctx.weight': 2}
    assert [g['names'] for g in flat['groups']] == fo.group_names()
    assert [(g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) for g in flat['groups']] == \
        [(1e-3, (0.9, 0.999), 1e-8, 0.0), (3e-4, (0.9, 0.999), 1e-8, 1e-5), (1e-5, (0.8, 0.99), 1e-8, 1e-5)]
    # the moments sit at their parameters' offsets whatever the numbering of the state was
    assert torch.equal(flat['exp_avg'], fo._m.cpu()) and torch.equal(flat['exp_avg_sq'], fo._v.cpu())
    back = util.flat_to_checkpoint(flat, model)
    assert back['param_group_names'] == fo.group_names()
    a, b = back['optimizer'], ck['optimizer']
    assert a['state'].keys() == b['state'].keys()
    for i in a['state']:
        assert float(a['state'][i]['step']) == float(b['state'][i]['step'])
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(a['state'][i][k], b['state'][i][k]), (i, k)
    for ga, gb in zip(a['param_groups'], b['param_groups']):
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params'):
            assert tuple(ga[k]) == tuple(gb[k]) if isinstance(ga[k], (tuple, list)) else ga[k] == gb[k], k
    # ... which a stock Adam with the same groups loads
    ref, _ = _stock(model, fo)
    ref.load_state_dict(back['optimizer'])
    # without the names a grouped state cannot be placed
    with pytest.raises(ValueError, match='param_group_names'):
        util.checkpoint_to_flat({k: v for k, v in ck.items() if k != 'param_group_names'}, model)
    # one group: the flat form as it always was
    plain = FusedAdam(model)
    flat1 = util.checkpoint_to_flat({'epoch': 0, 'state_dict': model.state_dict(), 'optimizer': plain.state_dict()}, model)
    assert 'groups' not in flat1 and 'param_group_names' not in util.flat_to_checkpoint(flat1, model)


# ---------------------------------------------------------------------------------------------------------------------------
# the constructor
# ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_errors():
    model, _, _ = _model()
    names = [n for n, _ in model.named_parameters()]
    with pytest.raises(ValueError, match='in no parameter group'):
        FusedAdam(model, param_groups=[dict(params=names[:-1])])                                   # an unlisted parameter
    with pytest.raises(ValueError, match='is in parameter groups'):
        FusedAdam(model, param_groups=[dict(params=names), dict(params=names[:1])])                # listed twice
    with pytest.raises(ValueError, match='is in parameter groups'):
        FusedAdam(model, param_groups=[dict(params=names + names[:1])])
    with pytest.raises(ValueError, match='at most 8'):
        FusedAdam(model, param_groups=[dict(params=[n]) for n in names[:8]] + [dict(params=names[8:])])      # nine groups
    with pytest.raises(ValueError, match='amsgrad'):
        FusedAdam(model, amsgrad=True)
    with pytest.raises(ValueError, match='amsgrad'):
        FusedAdam(model, param_groups=[dict(params=names, amsgrad=True)])
    with pytest.raises(ValueError, match='Invalid learning rate'):
        FusedAdam(model, lr=-1e-3)
    with pytest.raises(ValueError, match='Invalid learning rate'):
        FusedAdam(model, param_groups=[dict(params=names[:3], lr=-1.0), dict(params=names[3:])])
    with pytest.raises(ValueError, match='Invalid beta parameter at index 0'):
        FusedAdam(model, param_groups=[dict(params=names, betas=(1.0, 0.999))])
    with pytest.raises(ValueError, match='Invalid beta parameter at index 1'):
        FusedAdam(model, betas=(0.9, -0.1))
    with pytest.raises(ValueError, match='Invalid epsilon'):
        FusedAdam(model, eps=-1e-8)
    with pytest.raises(ValueError, match='Invalid weight_decay'):
        FusedAdam(model, param_groups=[dict(params=names, weight_decay=-1.0)])
    with pytest.raises(ValueError, match='no parameter of the model'):
        FusedAdam(model, param_groups=[dict(params=names + ['nobody.weight'])])
    with pytest.raises(ValueError, match='need device_hyper'):
        FusedAdam(model, param_groups=[dict(params=names[:3]), dict(params=names[3:])], device_hyper=False)
    # torch raises the same for the same values
    for kw in (dict(lr=-1e-3), dict(betas=(1.0, 0.999)), dict(eps=-1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            torch.optim.Adam(list(model.parameters()), **kw)
    # eight groups are fine; parameter objects and names may be mixed; what a group omits is the constructor's
    pd = dict(model.named_parameters())
    fo = FusedAdam(model, lr=2e-4, eps=1e-7, param_groups=[dict(params=[pd[n]], lr=1e-3) for n in names[:7]] + [dict(params=names[7:])])
    assert len(fo.param_groups) == 8 and fo.device_hyper
    assert fo.param_groups[0]['lr'] == 1e-3 and fo.param_groups[7]['lr'] == 2e-4 and all(g['eps'] == 1e-7 for g in fo.param_groups)
    assert fo.group_membership() == tuple(range(7)) + (7,) * 31
    with pytest.raises(RuntimeError, match='fixed at construction'):
        fo.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3))]))
    # device_hyper: None = on with more than one group, off with one; True is allowed with one
    assert not FusedAdam(model).device_hyper and not FusedAdam(model, param_groups=None).device_hyper
    assert not FusedAdam(model, param_groups=[dict(params=names)]).device_hyper
    assert FusedAdam(model, device_hyper=True).device_hyper and FusedAdam(model, param_groups=[dict(params=names)], device_hyper=True).device_hyper


def test_param_groups_is_torchs_list_and_a_scheduler_moves_it():
    model, _, _ = _model()
    fo = _grouped(model)
    sched = torch.optim.lr_scheduler.LambdaLR(fo, lambda s: 0.5 ** s)
    fo._opt_called = True
    sched.step()
    assert [g['lr'] for g in fo.param_groups] == [5e-4, 1.5e-4, 5e-6]
    assert [r[0] for r in fo.hyper_rows()] == [5e-4, 1.5e-4, 5e-6]
    for g in fo.param_groups:
        g['lr'] = 1e-2
    assert [r[0] for r in fo.hyper_rows()] == [1e-2] * 3
    fo.param_groups[1]['lr'] = -1.0
    with pytest.raises(ValueError, match='Invalid learning rate'):
        fo.hyper_rows()


# ---------------------------------------------------------------------------------------------------------------------------
# the recorded step's key
# ---------------------------------------------------------------------------------------------------------------------------
def test_recording_key_under_device_hyper():
    model, _, _ = _model()
    by_value = FusedAdam(model, lr=3e-5, weight_decay=1e-5)
    assert RecordedTrainStep.hyper_key(by_value) == (3e-5, (0.9, 0.999), 1e-8, 1e-5, 1.0)            # today's key
    one = FusedAdam(model, lr=3e-5, weight_decay=1e-5, device_hyper=True)
    k1 = RecordedTrainStep.hyper_key(one)
    assert k1 == (('device_hyper', (0,) * 38), 1.0)
    one.param_groups[0]['lr'] = 1e-3
    one.param_groups[0]['weight_decay'] = 0.0
    one.param_groups[0]['betas'] = (0.5, 0.9)
    one.param_groups[0]['eps'] = 1e-6
    assert RecordedTrainStep.hyper_key(one) == k1                  # the values are not in the key ...
    fo = _grouped(model)
    k3 = RecordedTrainStep.hyper_key(fo)
    assert k3[0] == ('device_hyper', fo.group_membership()) and k3 != k1          # ... the membership is
    one.device_hyper = False
    assert RecordedTrainStep.hyper_key(one) == (1e-3, (0.5, 0.9), 1e-6, 0.0, 1.0)             # switching it is another key
    # frozen parameters and clipping extend the key as they always did
    next(iter(model.parameters())).requires_grad_(False)
    assert RecordedTrainStep.hyper_key(fo)[:2] == k3 and len(RecordedTrainStep.hyper_key(fo)) == 3
    fo.max_grad_norm = 1.0
    assert RecordedTrainStep.hyper_key(fo)[-1] == ('max_grad_norm', 1.0)
    from lirec_amd import train
    assert repr(k3[0]) in train._flag_key(_grouped(_model()[0]))


def test_training_checks_scheduler_every():
    from lirec_amd import train
    with pytest.raises(ValueError, match='scheduler_every'):
        train.training(None, model=None, loss=None, optimizer=None, scheduler_every='sometimes')
