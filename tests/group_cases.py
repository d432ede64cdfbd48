"""Cases and yardsticks of the parameter-group tests (tests/test_host_groups.py, tests/test_gpu_groups.py,
tests/test_gpu_groups_parallel.py) -- not a test module.

The grouped update is adam_cases' update applied range by range: range r = (offset, length, lag, group) of the flat buffers is
updated with the five hyper-parameters of row `group` and the step max(t - lag, 1).  `ref64` is adam_cases.ref64 applied that
way, `ref32` adam_cases.ref32 (the bias corrections in double, cast: what the kernels do whether the step comes by value or from
the device); the bounds are adam_cases.bounds, unchanged.  tests/test_host_groups.py shows ref64 equal to torch.optim.Adam in
float64 with the same groups, and ref32 inside the bounds for every case the GPU file runs.

The kernel cases: ONE flat buffer with ranges of lengths 1, 3, 4, 5, 1023, 1024, 1025 and 4099 (a block edge on both sides,
scalar tails, one range of five blocks), GUARD words between them, dealt alternately to three groups whose rows are the first three
of adam_cases.HYPERS; lags 0 and 2 alternate; global steps 1, 3 and 1000.  One grad_scale per launch (0.125); gradients of
magnitude 1 -- with it |g gs| ~ 0.1 is far from every |wd p| <= 1e-3, the regime in which the bound on p' is not sound
(tests/test_host_clip.py, coefficient 2^-20): no case had to be left out for it.  A clipped launch: coefficient 0.37."""
import numpy as np

import adam_cases as AC
import clip_cases as CC

DIMS = dict(text_dim=24, visual_dim=32, track_dim=32)          # the `small` model of tests/host_dryrun.py
JOINT, B, T, R = 16, 4, 6, 3
N_CLASSES, N_RELS = 11, 5

LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
GUARD = 8                                                      # words between two ranges (and in front of the first)
STEPS = [1, 3, 1000]
GRAD_SCALE = 0.125
MAG = 1.0
COEF = 0.37
ROWS = [tuple(AC.HYPERS[i][:5]) for i in range(3)]             # (lr, beta1, beta2, eps, weight_decay) of groups 0, 1, 2
ROWS_B = [(2e-3, .8, .99, 1e-6, 1e-4), (5e-4, .95, .999, 1e-8, 0.0), (1e-4, .9, .9, 1e-8, 1e-3)]     # "other values" for the re-write
P_GUARD, M_GUARD, V_GUARD, G_GUARD = 7.25, -3.5, 11.0, 1e30    # what the guard words hold (a gradient guard that is USED shows)


def ranges():
    """[(offset, length, lag, group)]: offsets multiples of 4, GUARD or more words apart; and the buffer's length"""
    out, at = [], GUARD
    for i, k in enumerate(LENGTHS):
        out.append((at, k, (0, 2)[i % 2], i % 3))
        at = (at + k + GUARD + 3) // 4 * 4
    return out, at


def effective_step(step, lag):
    return max(step - lag, 1)


def hyper_of(row, grad_scale):
    return AC.hyper32(tuple(row) + (grad_scale,))


def build(step):
    """fp32 (p, g, m, v) of the kernel case at global step `step`, guards filled, and the ranges"""
    rs, n = ranges()
    p, g, m, v = (np.full(n, x, np.float32) for x in (P_GUARD, G_GUARD, M_GUARD, V_GUARD))
    for i, (o, k, lag, grp) in enumerate(rs):
        s = AC.make_state(AC.Case(grp, step, MAG), k, offset=i)
        for buf, x in zip((p, g, m, v), s):
            buf[o:o + k] = x
    return (p, g, m, v), rs


def inside(rs, n):
    mask = np.zeros(n, bool)
    for o, k, _, _ in rs:
        mask[o:o + k] = True
    return mask


def ref64(p, g, m, v, rs, step, rows, grad_scale, coef=1.0):
    """adam_cases.ref64 range by range: (p', m', v', bound_p, bound_m, bound_v), float64 arrays of the buffers' length; outside
    the ranges the values are the inputs and the bounds 0.  `coef`: the fp32 clip coefficient (clip_cases: the definition is the
    update of g * coef32)."""
    f = lambda a: np.asarray(a, np.float64).copy()
    pn, mn, vn = f(p), f(m), f(v)
    bp, bm, bv = (np.zeros(len(pn)) for _ in range(3))
    for o, k, lag, grp in rs:
        sl = slice(o, o + k)
        gg = g[sl] if coef == 1.0 else CC.scaled_g(np.asarray(g[sl]), coef)
        a, b_, c, G, A, V = AC.ref64(p[sl], gg, m[sl], v[sl], effective_step(step, lag), hyper_of(rows[grp], grad_scale))
        pn[sl], mn[sl], vn[sl] = a, b_, c
        bp[sl], bm[sl], bv[sl] = AC.bounds(p[sl], m[sl], G, A, V)
    return pn, mn, vn, bp, bm, bv


def ref32(p, g, m, v, rs, step, rows, grad_scale, coef=1.0):
    """the fp32 restatement range by range (the scale gs32 * coef32 rounded to fp32 once, as the clipped kernels form it)"""
    pn, mn, vn = (np.asarray(a, np.float32).copy() for a in (p, m, v))
    for o, k, lag, grp in rs:
        sl = slice(o, o + k)
        h = hyper_of(rows[grp], grad_scale)
        a, b_, c = CC.ref32(p[sl], g[sl], m[sl], v[sl], effective_step(step, lag), h, coef) if coef != 1.0 else \
            AC.ref32(p[sl], g[sl], m[sl], v[sl], effective_step(step, lag), h)
        pn[sl], mn[sl], vn[sl] = a, b_, c
    return pn, mn, vn


def use_of_bounds(got, p, g, m, v, rs, step, rows, grad_scale, coef=1.0):
    """[worst |got - ref64| / bound for p', m', v'] over the elements of the ranges"""
    ref = ref64(p, g, m, v, rs, step, rows, grad_scale, coef)
    mask = inside(rs, len(ref[0]))
    return [float((np.abs(np.asarray(x, np.float64) - r)[mask] / b[mask]).max()) for x, r, b in zip(got, ref[:3], ref[3:])]


# -- FusedAdam: the three groups of the issue ---------------------------------------------------------------------------------
GROUP_HYPERS = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-4), dict(lr=1e-5, betas=(0.8, 0.99))]


def three_groups(model):
    """all biases | the heads' and the gate's weights | the embeddings' weights, as lists of parameter names"""
    names = [n for n, _ in model.named_parameters()]
    heads = ('out_ints', 'out_ctx', 'gate')
    members = [[n for n in names if n.endswith('.bias')],
               [n for n in names if not n.endswith('.bias') and model.param_group_of(n) in heads],
               [n for n in names if not n.endswith('.bias') and model.param_group_of(n) not in heads]]
    assert all(members) and sum(len(x) for x in members) == len(names)
    return [dict(h, params=x) for h, x in zip(GROUP_HYPERS, members)]


def rows_of(optim):
    """(lr, beta1, beta2, eps, weight_decay) of every group of an optimiser, as param_groups has them"""
    return [(g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay']) for g in optim.param_groups]


def model_ranges(model, optim):
    """[(offset, length, lag, group)] of the model's flat layout, one range per TRAINABLE parameter (no merging: the per-element
    yardstick of a whole FusedAdam step)"""
    mem = dict(zip([n for n, _ in model.named_parameters()], optim.group_membership()))
    return [(model._offsets[n][0], model._offsets[n][1], optim._lag.get(n, 0), mem[n])
            for n, p in model.named_parameters() if p.requires_grad]
