"""The flag matrix itself (tests/flag_matrix_cases.py), checked on the host: its rows cover what they claim to cover, its factors
are the flags ``lirec_amd.config`` ships, and every flag of the build-side block of ``defaults()`` carries a decision -- a factor
of the matrix, or an entry of EXCLUDED with its reason.  The device runs are tests/test_gpu_flag_matrix.py."""
import inspect
import itertools
import re

import flag_matrix_cases as FM
from lirec_amd import config


def _rows():
    return {rid: FM.row(rid) for rid, _ in FM.ROWS}


def test_rows_are_well_formed():
    ids = [rid for rid, _ in FM.ROWS]
    assert len(set(ids)) == len(ids)
    for rid, vals in FM.ROWS:
        assert len(vals) == len(FM.FACTORS), rid
        for f, v in zip(FM.FACTORS, vals):
            assert v in FM.VALUES[f], (rid, f, v)
    assert len({vals for _, vals in FM.ROWS}) == len(FM.ROWS), 'two rows are the same row'


def test_default_row_is_defaults():
    d, r = config.defaults(), FM.row('default')
    for f in FM.FLAGS:
        assert r[f] is d[f], f
        assert FM.VALUES[f][0] is d[f], f
    # (the storage factor's default is to_device_batch's: an fp32 block)
    from lirec_amd.data import to_device_batch
    import torch
    assert inspect.signature(to_device_batch).parameters['feature_dtype'].default is torch.float32
    assert r[FM.STORAGE] == 'f32' == FM.VALUES[FM.STORAGE][0]


def test_every_flag_factor_is_a_boolean_default():
    d = config.defaults()
    for f in FM.FLAGS:
        assert f in d, f + ' is no field of config.defaults()'
        assert isinstance(d[f], bool), (f, type(d[f]))
    assert FM.STORAGE not in d


def test_every_single_flip_has_its_row():
    base, rows = FM.row('default'), _rows()
    for f in FM.FACTORS:
        want = dict(base)
        want[f] = FM.VALUES[f][1]
        assert rows.get(f) == want, 'no row flips %s alone' % f
        assert FM.refusal(rows[f]) is None and f not in FM.moot(rows[f]), f + ': its single flip takes no effect'


def test_rows_cover_every_pair_that_can_take_effect():
    req = FM.pairs_required()
    got = set()
    for r in _rows().values():
        got |= FM.pairs_covered(r)
    missing = sorted(req - got, key=str)
    assert not missing, '%d of %d pairs uncovered: %s' % (len(missing), len(req), missing[:8])
    # the requirement is not empty talk: all four value pairs of two factors without a moot rule between them, and of a factor
    # with the one that can make it moot only the pairs in which it is in force
    for a, b in (('compact_ctx_rows', 'h1_sign_bits'), ('wgrad_side_stream', 'adam_on_side_stream'), ('defer_side_join', 'fuse_dw1_adam')):
        for va, vb in itertools.product(FM.VALUES[a], FM.VALUES[b]):
            assert (a, va, b, vb) in req, (a, va, b, vb)
    assert ('layer1_planes', True, 'fuse_dw1_adam', False) in req and ('layer1_planes', False, 'fuse_dw1_adam', False) not in req
    assert ('gate_stage_on_side', False, 'wgrad_side_stream', False) not in req
    assert ('layer1_planes', False, FM.STORAGE, 'q32') not in req


def test_effective_and_refusals():
    rows = _rows()
    for rid, r in rows.items():
        e = FM.effective(r)
        assert set(e) == set(FM.FACTORS)
        for f in FM.FLAGS:
            assert e[f] in (r[f], False), (rid, f)           # (a rule only ever takes a feature out of force)
        assert e['gate_stage_on_side'] == (r['gate_stage_on_side'] and r['wgrad_side_stream'] and r['gate_q32'])
        assert e['fuse_dw1_adam'] == (r['fuse_dw1_adam'] and r['layer1_planes'])
        assert e['defer_side_join'] == r['defer_side_join'] and not FM.effective(r, overwrite=False)['defer_side_join']
    # the rows that are refused are the listed ones, and the rule predicts them
    assert {rid for rid, r in rows.items() if FM.refusal(r) is not None} == set(FM.REFUSALS)
    for rid, msg in FM.REFUSALS.items():
        assert FM.refusal(rows[rid]) == msg
    # the message is the model's
    from lirec_amd import model as M
    assert FM.Q32_WITHOUT_PLANES in inspect.getsource(M._HotPathModule._stage_plain)


def test_numeric_classes():
    classes = {FM.numeric_class(r) for r in _rows().values()}
    assert len(classes) <= 8
    assert FM.numeric_class(FM.row('default')) == (True, True, True)


def _build_side_flags():
    """the fields of defaults() below the line `# build-side additions`, in order"""
    src = inspect.getsource(config.defaults)
    assert src.count('# build-side additions') == 1
    tail = src.split('# build-side additions', 1)[1]
    first = re.search(r'^\s*(\w+)=', tail, re.M).group(1)
    keys = list(config.defaults())
    return keys[keys.index(first):]


def undecided(factors, excluded):
    d = config.defaults()
    return [k for k in _build_side_flags() if isinstance(d[k], (bool, str)) and k not in factors and k not in excluded]


def test_every_build_side_flag_is_a_factor_or_excluded_with_a_reason():
    d, side = config.defaults(), _build_side_flags()
    assert side[0] == 'dp_shard_eval' and 'h1_sign_bits' in side and 'joint_dim' not in side
    assert not undecided(FM.FLAGS, FM.EXCLUDED), 'flags without a decision: %s' % undecided(FM.FLAGS, FM.EXCLUDED)
    assert not set(FM.FLAGS) & set(FM.EXCLUDED)
    for k, why in FM.EXCLUDED.items():
        assert k in side, k + ' is excluded but is no build-side field of defaults()'
        assert isinstance(why, str) and len(why) > 10, k
    # the check bites: a factor taken out of both lists is reported
    assert undecided([f for f in FM.FLAGS if f != 'h1_sign_bits'], FM.EXCLUDED) == ['h1_sign_bits']
    assert undecided(FM.FLAGS, {k: v for k, v in FM.EXCLUDED.items() if k != 'record_block_store'}) == ['record_block_store']


def test_shapes_run_the_rows_the_matrix_names():
    ids = {rid for rid, _ in FM.ROWS}
    for s, (recipe, B, T, R, rows, recorded) in FM.SHAPES.items():
        assert set(rows) <= ids and rows[0] == 'default', s
    assert set(FM.SHAPES['S1'][4]) == ids, 'the whole matrix runs at S1'
    assert set(FM.SHAPES['S5'][4]) == {'default'} | set(FM.FACTORS)
    assert [s for s, spec in FM.SHAPES.items() if spec[5]] == ['S1', 'S4', 'S5']
    assert len(FM.CASES) == len(set(FM.CASES))
