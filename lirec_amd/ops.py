"""Thin tensor-level wrappers over the C ABI (include/lirec_hip.h).

Every function takes CUDA(HIP) fp32/int32 torch tensors, passes raw device
pointers plus the current torch stream, and checks the status code.  Torch is
only the owner of device memory and streams here; all arithmetic happens in
the HIP kernels.  CPU tensors are rejected: there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import threading

import torch

from . import _lib
from ._lib import (CLIP_WEIGHT_NORMS, ClipWeights, Dropout, FusedAdamArgs, EmbedBwdArgs, EmbedDxArgs, EmbedDxIndexedArgs, EmbedFwdArgs, EvalArgs,
                   EvalTopkArgs, LinearBwdArgs, LinearFwdArgs, LirecError, MarginLossArgs, Pieces, PredictArgs, RowSel, check, lib)


class _ThreadCell(threading.local):
    """one value per host thread, addressed as cell[0] (the recorder and the library contexts are per thread too)"""
    value = None

    def __getitem__(self, i):
        return self.value

    def __setitem__(self, i, v):
        self.value = v


_stream_override = _ThreadCell()  # raw stream handle every call of this thread uses instead of torch's current stream


def _stream():
    # (torch.cuda.current_stream() builds a Stream object and resolves the device three times: ~10 us a call,
    #  eight calls a step; the raw getter is one C call)
    h = _stream_override[0]
    if h is not None:
        return h
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def current_stream_handle():
    """Raw handle (ctypes void*) of the stream the next library call would use."""
    return _stream()


_keep = _ThreadCell()      # while a step is being recorded: every tensor the hot path allocates is appended (kept alive)


def new(*shape, **kw):
    """``torch.empty`` for the hot path's activations / scratch: under ``keep_allocations()`` the tensor stays alive for
    as long as the recorded command list that refers to its address."""
    t = torch.empty(*shape, **kw)
    if _keep[0] is not None:
        _keep[0].append(t)
    return t


def new_like(x):
    t = torch.empty_like(x)
    if _keep[0] is not None:
        _keep[0].append(t)
    return t


def keep(t):
    """Register a tensor torch made (a converted label / mask copy) with the active ``keep_allocations()``: a recorded command list
    carries its ADDRESS, so it must live as long as the list (it used to be freed at the end of the recording call, and the list
    read whatever the allocator put there next).  Returns ``t``."""
    if t is not None and _keep[0] is not None and torch.is_tensor(t):
        _keep[0].append(t)
    return t


class keep_allocations:
    def __enter__(self):
        self._prev, _keep[0] = _keep[0], []
        return _keep[0]

    def __exit__(self, *exc):
        _keep[0] = self._prev
        return False


class on_stream:
    """``with ops.on_stream(handle):`` -- library calls inside use that raw stream (no torch stream switch: the
    torch.cuda.stream() context manager costs ~20 us a time, three times a backward)."""

    def __init__(self, handle):
        self.handle, self._prev = handle, None

    def __enter__(self):
        self._prev = _stream_override[0]
        _stream_override[0] = self.handle
        return self

    def __exit__(self, *exc):
        _stream_override[0] = self._prev
        return False


def stream_wait(waiter, signaller):
    """``waiter`` (raw handle) waits for everything enqueued on ``signaller`` so far."""
    check(lib().lirec_stream_wait(waiter, signaller), 'lirec_stream_wait')


def stream_wait_many(waiters, signaller):
    """every stream of ``waiters`` (raw handles, at most four) waits for everything enqueued on ``signaller`` so far -- one
    event record for all of them"""
    arr = (C.c_void_p * len(waiters))(*[w.value if isinstance(w, C.c_void_p) else w for w in waiters])
    check(lib().lirec_stream_wait_many(arr, len(waiters), signaller), 'lirec_stream_wait_many')


def zero_(t):
    """Asynchronous memset of a contiguous device tensor on the current stream (recordable, unlike ``t.zero_()``)."""
    assert t.is_contiguous()
    check(lib().lirec_memset_zero(_p(t), t.numel() * t.element_size(), _stream()), 'lirec_memset_zero')
    return t


class CommandList:
    """Launches recorded between ``record_begin()`` and ``CommandList.end()`` (include/lirec_hip.h, "Command lists")."""

    def __init__(self, handle):
        self.handle = handle
        self.size = int(lib().lirec_cmdlist_size(handle))

    @staticmethod
    def begin():
        check(lib().lirec_record_begin(), 'lirec_record_begin')

    @staticmethod
    def mark() -> int:
        return int(lib().lirec_record_mark())

    @staticmethod
    def end():
        h = C.c_void_p()
        check(lib().lirec_record_end(C.byref(h)), 'lirec_record_end')
        return CommandList(h)

    lag = None        # diagnostics: (command index, ticks of the 100 MHz clock) -- that command's stream is held back in front of it

    def replay(self, begin: int = 0, end: int = -1):
        if self.lag is not None:
            check(lib().lirec_cmdlist_replay_lagged(self.handle, begin, end, int(self.lag[0]), int(self.lag[1])), 'lirec_cmdlist_replay_lagged')
            return
        check(lib().lirec_cmdlist_replay(self.handle, begin, end), 'lirec_cmdlist_replay')

    def command(self, i: int):
        """(stream handle, kind) of command i: kind 0 launch / memset, 1 stream wait (its signalling stream), 2 profiling bracket"""
        s, k = C.c_void_p(), C.c_int32()
        check(lib().lirec_cmdlist_command(self.handle, int(i), C.byref(s), C.byref(k)), 'lirec_cmdlist_command')
        return s.value, int(k.value)

    def destroy(self):
        if self.handle is not None:
            lib().lirec_cmdlist_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _p(t):
    """device pointer of a tensor (None -> NULL)"""
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.LirecError('lirec ops need device tensors (got a CPU tensor): the HIP path has no CPU fallback')
    return t.data_ptr()


def _f32c(t):
    assert t.dtype == torch.float32 and t.stride(-1) == 1, (t.dtype, t.stride())
    return t


class Q32Block:
    """A feature matrix stored as q32b on the device (include/lirec_hip.h: blocked bf16 hi / lo, the fp32 footprint) -- the storage
    layer 1 reads without a staging pass.  ``shape`` is the logical fp32 shape ((..., D), the leading dims flattened to rows),
    ``data`` the uint8 buffer.

    A batch of a RESIDENT BLOCK STORE (lirec_amd.blockstore) is such a block with ``clip_ids``: ``data`` is then the whole store
    (``store_rows`` rows, ``rows_per_clip`` consecutive ones per sample), ``shape`` the BATCH's ((B, ..., D)) and ``clip_ids`` the
    int32 device tensor [B] of the samples the batch is made of -- carried through ``view()``, handed to the library by the forward
    call (lirec_set_feature_rows); no row is copied."""
    dtype = 'q32'

    def __init__(self, data, shape, planes=2, k64=False, clip_ids=None, rows_per_clip=0, store_rows=0):
        """``planes`` = 1: q16b -- the values rounded to bf16, one plane, half the footprint (``to_q16b``; dtype 'q16');
        ``k64``: the same values as q16c (64-column blocks: ``to_q16c``) -- the storage of the single-pass mode (gemm mode 3)"""
        self.data, self.shape, self.device, self.planes, self.k64 = data, tuple(shape), data.device, int(planes), bool(k64)
        assert not self.k64 or self.planes == 1
        if self.planes == 1:
            self.dtype = 'q16'
        self.clip_ids, self.rows_per_clip, self.store_rows = clip_ids, int(rows_per_clip), int(store_rows)
        if clip_ids is not None:
            assert self.planes == 2 and clip_ids.dtype == torch.int32 and clip_ids.is_cuda and clip_ids.is_contiguous()

    def feature_rows(self):
        """the lirec_feature_rows of a block-store batch (None for a block that is its own storage)"""
        if self.clip_ids is None:
            return None
        fr = _lib.FeatureRows(self.clip_ids.data_ptr(), self.clip_ids.numel(), self.rows_per_clip, self.store_rows)
        fr._refs = (self.clip_ids, self.data)
        return fr

    @property
    def x_q32(self):
        """lirec_embed_fwd_args::x_q32 of this storage"""
        return 3 if self.k64 else (2 if self.planes == 1 else 1)

    def view(self, *shape):
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        n = 1
        for d in self.shape:
            n *= d
        shape = list(shape)
        if -1 in shape:
            k = 1
            for d in shape:
                k *= d if d != -1 else 1
            shape[shape.index(-1)] = n // k
        return Q32Block(self.data, shape, self.planes, self.k64, self.clip_ids, self.rows_per_clip, self.store_rows)

    def data_ptr(self):
        return self.data.data_ptr()

    def dim(self):
        return len(self.shape)

    @property
    def is_cuda(self):
        return self.data.is_cuda


def to_q32b(t, out=None):
    """fp32 device tensor (..., D), D % 32 == 0 -> ``Q32Block`` (lirec_to_q32b; rows padded to 32 with zero rows).  ``out``: a
    uint8 buffer of at least ``lirec_q32b_bytes(rows, D)`` bytes to write into (256-byte aligned)."""
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    D = t.shape[-1]
    rows = t.numel() // D
    need = max(int(lib().lirec_q32b_bytes(rows, D)), 256)
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=t.device)
    assert out.dtype == torch.uint8 and out.is_cuda and out.numel() >= need and out.data_ptr() % 256 == 0
    check(lib().lirec_to_q32b(_p(t), D, rows, D, _p(out), _stream()), 'lirec_to_q32b')
    return Q32Block(out, t.shape)


def q32b_write_rows(src, dst, row0, dst_rows):
    """Rows of ``src`` (fp32 or float64 device tensor (..., D), contiguous) -> storage rows [row0, row0 + rows) of the q32b matrix of
    ``dst_rows`` x D in the uint8 buffer ``dst`` (lirec_q32b_write_rows): the halves ``to_q32b`` writes for the same values -- a
    float64 value through fp32 first --, no other row touched."""
    assert src.is_cuda and src.dtype in (torch.float32, torch.float64) and src.is_contiguous()
    assert dst.dtype == torch.uint8 and dst.is_cuda and dst.is_contiguous()
    D = src.shape[-1]
    rows = src.numel() // D if D else 0
    assert dst.numel() >= int(dst_rows) * D * 4, (dst.numel(), dst_rows, D)
    if rows == 0:
        return
    check(lib().lirec_q32b_write_rows(_p(src), int(src.dtype == torch.float64), D, rows, D, _p(dst), int(row0), int(dst_rows), _stream()),
          'lirec_q32b_write_rows')


def to_q16b(t, out=None, k64=False):
    """fp32 (or bf16) device tensor (..., D), D % 32 == 0 -> ``Q32Block(planes=1)``: every value rounded to bf16 and stored blocked
    (lirec_to_q16b) -- "bf16 feature storage" in the layout the persistent layer-1 kernels gather their rows from.  ``k64``: as q16c
    (lirec_to_q16c, D % 64 == 0), the layout of the single-pass mode."""
    if t.dtype == torch.bfloat16:
        t = t.float()
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    D = t.shape[-1]
    rows = t.numel() // D
    need = max(int(lib().lirec_q16b_bytes(rows, D)), 256)
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=t.device)
    assert out.dtype == torch.uint8 and out.is_cuda and out.numel() >= need and out.data_ptr() % 256 == 0
    if k64:
        check(lib().lirec_to_q16c(_p(t), D, rows, D, _p(out), _stream()), 'lirec_to_q16c')
    else:
        check(lib().lirec_to_q16b(_p(t), D, rows, D, _p(out), _stream()), 'lirec_to_q16b')
    return Q32Block(out, t.shape, planes=1, k64=k64)


def to_q16c(t, out=None):
    return to_q16b(t, out=out, k64=True)


def to_q16(t, out=None):
    """bf16 feature storage in the blocked layout of the GEMM core IN FORCE: q16b for the split-precision core, q16c for the
    single-pass mode (each mode refuses the other's layout -- convert under the mode the batch will be used with)"""
    return to_q16b(t, out=out, k64=get_gemm_mode() == 3)


def make_dropout(seed: int, p: float, site: int = 0, site2: int = 0, seed_dev=None) -> Dropout:
    """``seed_dev``: optional device int64[1] tensor whose value the kernels add to ``seed`` (graph replay)."""
    return Dropout(int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), int(site), int(site2),
                   None if seed_dev is None else seed_dev.data_ptr())


class Segments:
    """Column segments of one head: (in_off, in_dim, out_dim) per branch."""

    def __init__(self, in_off, in_dim, out_dim):
        self.in_off, self.in_dim, self.out_dim = list(in_off), list(in_dim), list(out_dim)
        self.n = len(self.in_off)
        assert 1 <= self.n <= _lib.MAX_SEG

    @property
    def width(self):
        return sum(self.out_dim)


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = v


def embed_fwd_args(X, ldx, sel, rows, J, segs: Segments, W1, b1, W2, b2, H1, Z2, ldz2, Tn, ldtn, epilogue, drop,
                   pool=None, planes=None, pieces=None, hbits=None, rows_staged=False, W1q=None):
    """``pool`` = (mask [n,R] fp32, R, clamp_zero, Hbar [n, nseg*J], fscale [n]) selects the pooled form.
    ``planes``: uint8 workspace of ``planes_bytes(...)`` bytes -> layer 1 runs on pre-split bf16 planes.
    ``pieces`` (with ``planes``): a ``make_pieces`` struct -- the rows are staged from the piece tables, X is not read.
    ``hbits`` (pooled form): uint8 buffer of ``hbits_bytes(rows, nseg * J)`` bytes -> the pooling pass leaves the sign bits of H1
    there; backward reads them instead of H1."""
    a = EmbedFwdArgs()
    a.rows_staged = int(bool(rows_staged))
    if W1q is not None:       # the first-layer weights kept as q32b (addresses; lirec_embed_fwd_args::W1q)
        _fill(a.W1q, [int(w) for w in W1q])
    _fill_head_common(a, X, ldx, sel, rows, J, segs, drop, pool, planes, pieces, hbits)
    _fill(a.W1, [_p(w) for w in W1]); _fill(a.b1, [_p(w) for w in b1])
    _fill(a.W2, [_p(w) for w in W2]); _fill(a.b2, [_p(w) for w in b2])
    a.H1, a.Z2, a.ldz2 = _p(H1), Z2, ldz2
    a.Tn, a.ldtn = Tn, ldtn
    a.epilogue = epilogue
    return a


def _fill_head_common(a, X, ldx, sel, rows, J, segs, drop, pool, planes, pieces, hbits):
    """what a head's forward and backward structs share: the feature block and its storage form, the row selector, the
    segments, the dropout stream, and the optional pooled / compact tuple, planes workspace, piece tables and sign bits"""
    if hbits is not None:
        a.hbits = _p(hbits)
    if pieces is not None:
        a.pieces = C.cast(C.pointer(pieces), C.c_void_p)
        a._pieces_ref = pieces
    if planes is not None:
        a.planes, a.planes_bytes = _p(planes), planes.numel() * planes.element_size()
    if pool is not None:
        mask, R, clamp, Hbar, fscale = pool[:5]
        a.mask, a.R, a.clamp_zero, a.Hbar, a.fscale = _p(mask), R, int(clamp), _p(Hbar), _p(fscale)
        if len(pool) > 5 and pool[5] is not None:          # compact form: (rowmap, cstart, count[, wts])
            a.rowmap, a.cstart, a.count = (_p(t) for t in pool[5][:3])
            a.wts = _p(pool[5][3]) if len(pool[5]) > 3 else None
    a.X, a.ldx = _p(X), ldx
    a.x_bf16 = int(X.dtype == torch.bfloat16)
    a.x_q32 = X.x_q32 if isinstance(X, Q32Block) else 0
    a._frows = X.feature_rows() if isinstance(X, Q32Block) else None     # (a block-store batch: armed by the forward call)
    _fill(a.in_off, segs.in_off); _fill(a.in_dim, segs.in_dim); _fill(a.out_dim, segs.out_dim)
    a.rows, a.nseg, a.J = rows, segs.n, J
    a.sel = RowSel(*sel)
    a.drop = drop


def _arm_feature_rows(*heads):
    """lirec_set_feature_rows for the forward call about to be made, when its heads read a block-store batch: the parts of the
    call that turn block rows into storage rows (0, 1, 4) -- parts 2 and 3 read no rows and take no setter.  The library consumes
    it in that call."""
    fr = getattr(heads[0], '_frows', None)
    if len({getattr(h, '_frows', None) is None for h in heads}) > 1:
        raise LirecError('the heads of one forward call must read the same feature block')
    if fr is not None and heads[0].parts in (0, 1, 4):
        check(lib().lirec_set_feature_rows(C.byref(fr)), 'lirec_set_feature_rows')


def embed_fwd(*args, **kw):
    a = kw['args'] if 'args' in kw else embed_fwd_args(*args, **kw)
    _arm_feature_rows(a)
    check(lib().lirec_embed_fwd(C.byref(a), _stream()), 'lirec_embed_fwd')


def embed_fwd2(a, b):
    """Both heads in one call (``a``, ``b`` from embed_fwd_args): their second layers share a grouped launch."""
    _arm_feature_rows(a, b)
    check(lib().lirec_embed_fwd2(C.byref(a), C.byref(b), _stream()), 'lirec_embed_fwd2')


def embed_fwd_heads(heads, parts=None):
    """The forward of one head (lirec_embed_fwd) or of two in one call (lirec_embed_fwd2): ``heads`` is a list of one or two
    embed_fwd_args structs, None entries are dropped and an empty list is a no-op.  ``parts``: run ``with_parts`` copies."""
    heads = [h if parts is None else with_parts(h, parts) for h in heads if h is not None]
    if heads:
        embed_fwd(args=heads[0]) if len(heads) == 1 else embed_fwd2(*heads)


def embed_bwd_heads(heads, parts=None):
    """The backward of one head (lirec_embed_bwd) or of two in one call (lirec_embed_bwd2); arguments as embed_fwd_heads."""
    heads = [h if parts is None else with_parts(h, parts) for h in heads if h is not None]
    if heads:
        embed_bwd(args=heads[0]) if len(heads) == 1 else embed_bwd2(*heads)


def embed_bwd_args(X, ldx, sel, rows, J, segs: Segments, W2, H1, dZ2, lddz2, dW1, db1, dW2, db2, workspace, drop,
                   pool=None, planes=None, parts=0, hbits=None, pieces=None, adam=None):
    """``H1`` may be None when ``hbits`` (the sign bits the forward call left) is given.  ``pieces``: the forward call's, when its
    rows were gathered from q32b piece tables.  ``adam``: a ``FusedAdamArgs`` struct -- the first-layer parameters' update folded into
    the weight-gradient reduce (lirec_embed_bwd_args::adam)."""
    a = EmbedBwdArgs()
    a.parts = int(parts)
    if adam is not None:
        a.adam = C.cast(C.pointer(adam), C.c_void_p)
        a._adam_ref = adam
    _fill_head_common(a, X, ldx, sel, rows, J, segs, drop, pool, planes, pieces, hbits)
    _fill(a.W2, [_p(w) for w in W2])
    a.H1, a.dZ2, a.lddz2 = (_p(H1) if H1 is not None else None), dZ2, lddz2
    _fill(a.dW1, [_p(w) for w in dW1]); _fill(a.db1, [_p(w) for w in db1])
    _fill(a.dW2, [_p(w) for w in dW2]); _fill(a.db2, [_p(w) for w in db2])
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel() * workspace.element_size()
    # the struct only holds raw pointers: keep what it points into alive for as long as the struct (or a with_parts copy) is
    a._refs = (X, H1, workspace, planes, pool, hbits)
    return a


def make_pieces(clip, track, index, text_dim, visual_dim, clip_rows=None, track_rows=None):
    """lirec_pieces from device tensors: clip table [n_clip, text+visual] fp32, track table [n_track, track_dim] fp32,
    index [..., 3] int32.  The tables may be ``Q32Block``s (``to_q32b``): layer 1 then gathers its rows from them through the
    index -- and, with ``clip_rows`` / ``track_rows`` (int32 lists), through those lists first (a store of all pieces)."""
    assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous()
    if isinstance(clip, Q32Block):
        assert isinstance(track, Q32Block) and clip.shape[1] == text_dim + visual_dim
        pc = Pieces(None, clip.shape[1], clip.shape[0] - 1, None, track.shape[1], track.shape[0] - 1, _p(index),
                    text_dim, visual_dim, track.shape[1])
        pc.clip_q, pc.track_q = _p(clip), _p(track)
        if clip_rows is not None:
            assert clip_rows.dtype == torch.int32 and track_rows.dtype == torch.int32 and clip_rows.is_cuda and track_rows.is_cuda
            pc.clip_rows, pc.track_rows = _p(clip_rows), _p(track_rows)
        pc._refs = (clip, track, index, clip_rows, track_rows)
        return pc
    assert clip.is_cuda and clip.dtype == torch.float32 and track.dtype == torch.float32
    assert clip.is_contiguous() and track.is_contiguous() and clip.shape[1] == text_dim + visual_dim
    # (both tables carry one extra zero row behind their pieces: the piece of a negative index, lirec_embed_dw1_indexed)
    return Pieces(_p(clip), clip.shape[1], clip.shape[0] - 1, _p(track), track.shape[1], track.shape[0] - 1, _p(index),
                  text_dim, visual_dim, track.shape[1])


def embed_l1_indexed(heads, pieces, zclips, ztrks):
    """Layer 1 of the given heads (EmbedFwdArgs) on the unique feature pieces (lirec_embed_l1_indexed)."""
    n = len(heads)
    hp = (C.POINTER(EmbedFwdArgs) * n)(*[C.pointer(h) for h in heads])
    zc = (C.c_void_p * n)(*[_p(z) for z in zclips])
    zt = (C.c_void_p * n)(*[_p(z) for z in ztrks])
    check(lib().lirec_embed_l1_indexed(hp, n, C.byref(pieces), zc, zt, _stream()), 'lirec_embed_l1_indexed')


def embed_dw1_indexed(heads, pieces, Ps, Ss):
    """First-layer weight gradients of the given heads (EmbedBwdArgs) from the unique pieces (lirec_embed_dw1_indexed)."""
    n = len(heads)
    hp = (C.POINTER(EmbedBwdArgs) * n)(*[C.pointer(h) for h in heads])
    pp = (C.c_void_p * n)(*[_p(z) for z in Ps])
    sp = (C.c_void_p * n)(*[_p(z) for z in Ss])
    check(lib().lirec_embed_dw1_indexed(hp, n, C.byref(pieces), pp, sp, _stream()), 'lirec_embed_dw1_indexed')


def fused_adam_args(p, g, m, v, n_params, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, step_dev=None, wq=None, wq_first=0):
    """``FusedAdamArgs`` (lirec_fused_adam): p, g, m, v flat fp32 device tensors of one layout; ``wq``: uint8 shadow buffer whose byte 0
    is the q32b form of the weights at element ``wq_first``."""
    for t in (p, g, m, v):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    a = FusedAdamArgs(_p(p), _p(g), _p(m), _p(v), _p(wq) if wq is not None else None, int(wq_first), p.numel(), int(n_params),
                int(step), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(grad_scale),
                None if step_dev is None else step_dev.data_ptr())
    a._refs = (p, g, m, v, wq, step_dev)
    return a


def with_parts(a, parts):
    """copy of an argument struct with another ``parts`` selection"""
    b = type(a).from_buffer_copy(a)
    b.parts = int(parts)
    b._refs = getattr(a, '_refs', None)
    b._pieces_ref = getattr(a, '_pieces_ref', None)
    b._adam_ref = getattr(a, '_adam_ref', None)
    b._frows = getattr(a, '_frows', None)
    return b


def embed_bwd(*args, **kw):
    a = kw['args'] if 'args' in kw else embed_bwd_args(*args, **kw)
    check(lib().lirec_embed_bwd(C.byref(a), _stream()), 'lirec_embed_bwd')


def embed_bwd2(a, b):
    check(lib().lirec_embed_bwd2(C.byref(a), C.byref(b), _stream()), 'lirec_embed_bwd2')


def embed_dx(heads, W1, dX):
    """Input-feature gradient (lirec_embed_dx): ``heads`` = the EmbedBwdArgs of the backward call that just ran (both heads in
    the order given to embed_bwd2, or the one head of embed_bwd), ``W1`` = per head the first-layer weights of its segments,
    ``dX`` = the contiguous (n, R+1, D) fp32 / bf16 device block to overwrite."""
    assert dX.is_cuda and dX.is_contiguous() and dX.dim() == 3 and dX.dtype in (torch.float32, torch.bfloat16)
    a = EmbedDxArgs()
    a.nh = len(heads)
    for h, (b, ws) in enumerate(zip(heads, W1)):
        a.heads[h] = C.pointer(b)
        _fill(a.W1[h], [_p(w) for w in ws])
    a.out_bf16 = int(dX.dtype == torch.bfloat16)
    a.dX, a.ldx = _p(dX), dX.shape[2]
    a.n, a.rp1, a.D = dX.shape[0], dX.shape[1], dX.shape[2]
    check(lib().lirec_embed_dx(C.byref(a), _stream()), 'lirec_embed_dx')


def embed_dx_indexed(heads, S, W1, pieces, dClip, dTrack):
    """Gradient of the piece tables (lirec_embed_dx_indexed): ``heads``, ``pieces`` and ``S`` = what the embed_dw1_indexed call
    that just ran was given, ``W1`` = per head the first-layer weights of its four segments, ``dClip`` / ``dTrack`` = contiguous
    fp32 device tensors of the tables' shapes (zero rows included) to overwrite."""
    for t in (dClip, dTrack):
        assert t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.dtype == torch.float32
    a = EmbedDxIndexedArgs()
    a.nh = len(heads)
    for h, (b, s, ws) in enumerate(zip(heads, S, W1)):
        a.heads[h] = C.pointer(b)
        a.S[h] = _p(s)
        _fill(a.W1[h], [_p(w) for w in ws])
    a.pieces = C.pointer(pieces)
    a.dClip, a.ld_clip = _p(dClip), dClip.shape[1]
    a.dTrack, a.ld_track = _p(dTrack), dTrack.shape[1]
    check(lib().lirec_embed_dx_indexed(C.byref(a), _stream()), 'lirec_embed_dx_indexed')


_MASK_DTYPES = {torch.float32: 0, torch.int64: 1, torch.float64: 2}


def compact_rows(mask, n, R, out=None):
    """(rowmap [n*R], cstart [n+1], count [1], wts [n*R]) device tensors for the rows with a non-zero mask.  ``mask`` is
    read in the dtype the loader delivers it (int64 ``rels_mask``; or fp32 / float64): no cast kernel;
    ``wts`` holds the mask value of every compact row as fp32 (what the pooling passes multiply by).  ``out``: such a tuple to
    write into again (same n, R)."""
    dev = mask.device
    assert mask.is_contiguous() and mask.numel() == n * R and mask.dtype in _MASK_DTYPES, (mask.dtype, mask.shape)
    if out is not None:
        rowmap, cstart, count, wts = out
        assert rowmap.numel() == n * R and cstart.numel() == n + 1
    else:
        rowmap = new(n * R, dtype=torch.int32, device=dev)
        cstart = new(2 * n + 1, dtype=torch.int32, device=dev)[:n + 1]      # (+ n ints of scratch behind it, see the header)
        count = new(1, dtype=torch.int32, device=dev)
        wts = new(n * R, dtype=torch.float32, device=dev)
    check(lib().lirec_compact_rows2(_p(mask), _MASK_DTYPES[mask.dtype], n, R, _p(rowmap), _p(cstart), _p(count), _p(wts),
                                    _stream()), 'lirec_compact_rows2')
    return rowmap, cstart, count, wts


def workspace_bytes(rows, nseg, J):
    return int(lib().lirec_workspace_bytes(rows, nseg, J))


def hbits_bytes(rows, W):
    """bytes of the sign-bit buffer of a pooled head (lirec_embed_fwd_args.hbits)"""
    return int(lib().lirec_hbits_bytes(int(rows), int(W)))


def planes_bytes(rows, dsum, J, gathered=False, bf16=False):
    """bytes of one head's `planes` workspace (staged feature rows -- none when they are ``gathered`` from q32b storage, one plane
    when the block is ``bf16`` --, first-layer weights, dropout keep bytes, row lists)"""
    return int(lib().lirec_planes_bytes(rows, dsum, J, 1 if bf16 else (2 if gathered else 0)))


def pool_fwd(Z2, ldz, mask, n, R, W, clamp, Tn, ldtn, E, lde, drop):
    check(lib().lirec_pool_fwd(_p(Z2), ldz, _p(mask), n, R, W, int(clamp), Tn, ldtn, E, lde, C.byref(drop), _stream()),
          'lirec_pool_fwd')


def pool_bwd(dP, lddp, mask, n, R, W, clamp, dZ2, lddz):
    check(lib().lirec_pool_bwd(dP, lddp, _p(mask), n, R, W, int(clamp), _p(dZ2), lddz, _stream()), 'lirec_pool_bwd')


def gate_ws_bytes(n, K, N):
    """bytes of the q32b workspace of the gate GEMMs (lirec_gate_fwd_ws / lirec_gate_bwd_ws)"""
    return int(lib().lirec_gate_ws_bytes(int(n), int(K), int(N)))


def gate_stage_weights(Wg, n, K, N, ws) -> bool:
    """Stage the gate's weights into ``ws`` on the current (library) stream; False when the q32b path does not apply."""
    rc = lib().lirec_gate_stage_weights(_p(Wg), n, K, N, _p(ws), ws.numel() * ws.element_size(), _stream())
    if rc == _lib.LIREC_EINVAL:
        return False
    check(rc, 'lirec_gate_stage_weights')
    return True


def gate_fwd(EE, ldee, Wg, bg, n, K, N, G, ldg, drop, ws=None, weights_staged=False):
    """``ws`` (uint8, ``gate_ws_bytes``): forward on staged q32b operands (wave-specialised kernel) when the shapes qualify; the
    same buffer must then be handed to ``gate_bwd``.  ``weights_staged``: ``gate_stage_weights`` has filled the weights' part."""
    if ws is not None:
        check(lib().lirec_gate_fwd_ws(_p(EE), ldee, _p(Wg), _p(bg), n, K, N, _p(G), ldg, C.byref(drop), _p(ws),
                                      ws.numel() * ws.element_size(), int(weights_staged), _stream()), 'lirec_gate_fwd_ws')
        return
    check(lib().lirec_gate_fwd(_p(EE), ldee, _p(Wg), _p(bg), n, K, N, _p(G), ldg, C.byref(drop), _stream()),
          'lirec_gate_fwd')


def gate_bwd(dZg, lddzg, EE, ldee, Wg, n, K, N, split, Tn, ldtn, dWg, dbg, dEE, lddee, acc_first, drop,
             site_ctx, site_ints, parts=0, ws=None, rows_staged=False):
    """``parts``: 0 both, 1 only dWg / dbg, 2 only dEE; with ``ws`` (the workspace the forward call staged Wg and EE into) also
    4 = stage the rows of dZg only, after which the other parts are called with ``rows_staged``."""
    if ws is not None:
        check(lib().lirec_gate_bwd_ws(_p(dZg), lddzg, _p(EE), ldee, _p(Wg), n, K, N, split, _p(Tn), ldtn, _p(dWg), _p(dbg),
                                      _p(dEE), lddee, int(acc_first), C.byref(drop), site_ctx, site_ints, int(parts), _p(ws),
                                      ws.numel() * ws.element_size(), int(rows_staged), _stream()), 'lirec_gate_bwd_ws')
        return
    check(lib().lirec_gate_bwd_parts(_p(dZg), lddzg, _p(EE), ldee, _p(Wg), n, K, N, split, _p(Tn), ldtn, _p(dWg), _p(dbg),
                                     _p(dEE), lddee, int(acc_first), C.byref(drop), site_ctx, site_ints, int(parts), _stream()),
          'lirec_gate_bwd_parts')


def linear_fwd(A, lda, W, b, n, K, N, Y, ldy):
    check(lib().lirec_linear_fwd(A, lda, _p(W), _p(b), n, K, N, _p(Y), ldy, _stream()), 'lirec_linear_fwd')


def linear_fwd_group(items):
    """items: (A, lda, W, b, n, K, N, Y, ldy) per head, as for linear_fwd; one grouped launch."""
    arr = (LinearFwdArgs * len(items))()
    for v, (A, lda, W, b, n, K, N, Y, ldy) in zip(arr, items):
        v.A, v.lda, v.W, v.b, v.Y, v.ldy, v.n, v.K, v.N = A, lda, _p(W), _p(b), _p(Y), ldy, n, K, N
    check(lib().lirec_linear_fwd_group(arr, len(items), _stream()), 'lirec_linear_fwd_group')


def linear_bwd_group(items, parts=0):
    """items: the argument tuples of linear_bwd, one per head; dW of all heads in one launch, dA likewise.
    ``parts``: 0 both, 1 only the weight gradients, 2 only the data gradients."""
    arr = (LinearBwdArgs * len(items))()
    for v, (dY, lddy, A, lda, W, n, K, N, dW, db, dA, ldda, mode, act, ldact, accumulate, drop) in zip(arr, items):
        v.dY, v.lddy, v.A, v.lda, v.W = _p(dY), lddy, A, lda, _p(W)
        v.dW, v.db, v.dA, v.ldda, v.act, v.ldact = _p(dW), _p(db), dA, ldda, act, ldact
        v.n, v.K, v.N, v.mode, v.accumulate, v.parts = n, K, N, mode, int(accumulate), int(parts)
        v.drop = drop
    check(lib().lirec_linear_bwd_group(arr, len(items), _stream()), 'lirec_linear_bwd_group')


def linear_bwd(dY, lddy, A, lda, W, n, K, N, dW, db, dA, ldda, mode, act, ldact, accumulate, drop):
    check(lib().lirec_linear_bwd(_p(dY), lddy, A, lda, _p(W), n, K, N, _p(dW), _p(db), dA, ldda, mode, act, ldact,
                                 int(accumulate), C.byref(drop), _stream()), 'lirec_linear_bwd')


_ARRIVE = {}


def _arrive_counter(dev):
    """The in-launch finalize's arrival counter: zero on entry, left zero by the kernel.  One per (device, stream): loss
    launches of one stream are ordered, launches in flight on two streams (a validation loss beside training) must not
    share tickets."""
    key = (dev.type, dev.index, current_stream_handle().value)
    if key not in _ARRIVE:
        _ARRIVE[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _ARRIVE[key]


def margin_loss(ints, rels, mem, w, y, r, g, sel, B, T, Cc, NR, margin, lymbda, max_neg, tr_correct,
                mask_inplace, rels_mean_valid, loader_types=False, sample=0, sample_seed=0, sample_seed_dev=None,
                want_probs=False, heads=None, back=None, divisors=None, y_stride=1, clip_weight=None, clip_weight_norm='sum',
                clip_loss=None):
    """Fused loss forward+backward.  ``ints`` [B*T, C] is modified in place when
    ``mask_inplace``.  Returns (loss[1], d_ints, d_rels|None, sel_out[B], probs[B,T]|None).
    ``sample``: 1 draws the positive track in the kernel (tr_cat_distr); 2 only computes probs / the draw (no loss).
    ``heads`` / ``back``: the whole K5 boundary call, lirec_heads_loss_fwd_bwd -- ``heads`` = linear_fwd_group items whose
    outputs ARE ``ints`` / ``rels``, ``back`` = linear_bwd_group items with the string 'ints' / 'rels' in place of dY (the
    gradient buffers are made here); heads forward, this loss and the heads' data gradients in one library call.
    ``divisors``: the data-parallel denominators of the batch means (lirec_margin_loss_args::batch_divisor) -- a pair of numbers
    (batch, labelled relationship rows; 0 = this batch's own) or a device float32[2] tensor the kernel reads.
    ``clip_weight`` / ``clip_weight_norm`` / ``clip_loss``: lirec_clip_weights -- a device [B] float32 or float64 tensor of per-clip
    weights (taken as given: not checked for sign or finiteness), 'sum' | 'count', and a device float32 [B, 2] tensor that receives
    the per-clip values (lymbda * li_b, lr_b); with neither, the unweighted export is called."""
    dev = ints.device
    probs_only = sample == 2
    cw = _clip_weights(clip_weight, clip_weight_norm, clip_loss, B, dev)
    d_ints = None if probs_only else new((B * T, Cc), dtype=torch.float32, device=dev)
    d_rels = new((B * T, NR), dtype=torch.float32, device=dev) if (rels is not None and not probs_only) else None
    loss = None if probs_only else new(1, dtype=torch.float32, device=dev)
    partial = None if probs_only else new(2 * B + 2, dtype=torch.float32, device=dev)
    sel_out = new(B, dtype=torch.int32, device=dev)
    probs = new((B, T), dtype=torch.float32, device=dev) if (want_probs or probs_only) else None
    a = MarginLossArgs()
    a.ints, a.ld_ints = _p(ints), ints.stride(0)
    a.rels, a.ld_rels = _p(rels), (rels.stride(0) if rels is not None else 0)
    a.mem, a.w, a.y, a.r, a.g, a.sel = _p(mem), _p(w), _p(y), _p(r), _p(g), _p(sel)
    a.d_ints, a.ld_dints = _p(d_ints), Cc
    a.d_rels, a.ld_drels = _p(d_rels), NR
    a.loss, a.partial, a.sel_out = _p(loss), _p(partial), _p(sel_out)
    a.B, a.T, a.C, a.NR = B, T, Cc, NR
    a.margin, a.lymbda = margin, lymbda
    a.max_neg, a.tr_correct, a.mask_inplace, a.rels_mean_valid = int(max_neg), int(tr_correct), int(mask_inplace), int(rels_mean_valid)
    a.loader_types = int(bool(loader_types))
    a.sample, a.sample_seed = int(sample), int(sample_seed) & 0xFFFFFFFFFFFFFFFF
    a.sample_seed_dev = _p(sample_seed_dev)
    a.probs_out = _p(probs)
    a.arrive = None if probs_only else _p(_arrive_counter(dev))
    _set_divisors(a, divisors, dev)
    a.y_stride = int(y_stride)
    if loader_types:
        assert all(t is None or t.dtype == torch.float64 for t in (mem, w)) and \
            all(t is None or t.dtype == torch.int64 for t in (y, r, g))
    else:
        assert all(t is None or t.dtype == torch.float32 for t in (mem, w)) and \
            all(t is None or t.dtype == torch.int32 for t in (y, r, g))
    if heads is None:
        if cw is None:
            check(lib().lirec_margin_loss(C.byref(a), _stream()), 'lirec_margin_loss')
        else:
            check(lib().lirec_margin_loss_weighted(C.byref(a), C.byref(cw), _stream()), 'lirec_margin_loss_weighted')
        return loss, d_ints, d_rels, sel_out, probs
    assert back is not None and len(back) == len(heads) and not probs_only
    fwd = (LinearFwdArgs * len(heads))()
    for v, (A, lda, W, b, n, K, N, Y, ldy) in zip(fwd, heads):
        v.A, v.lda, v.W, v.b, v.Y, v.ldy, v.n, v.K, v.N = A, lda, _p(W), _p(b), _p(Y), ldy, n, K, N
    bwd = (LinearBwdArgs * len(back))()
    for v, (dY, lddy, A, lda, W, n, K, N, dW, db, dA, ldda, mode, act, ldact, accumulate, drop) in zip(bwd, back):
        dYt = {'ints': d_ints, 'rels': d_rels}[dY]
        v.dY, v.lddy, v.A, v.lda, v.W = _p(dYt), lddy, A, lda, _p(W)
        v.dW, v.db, v.dA, v.ldda, v.act, v.ldact = _p(dW), _p(db), dA, ldda, act, ldact
        v.n, v.K, v.N, v.mode, v.accumulate, v.parts = n, K, N, mode, int(accumulate), 2
        v.drop = drop
    if cw is None:
        check(lib().lirec_heads_loss_fwd_bwd(fwd, bwd, len(heads), C.byref(a), _stream()), 'lirec_heads_loss_fwd_bwd')
    else:
        check(lib().lirec_heads_loss_fwd_bwd_weighted(fwd, bwd, len(heads), C.byref(a), C.byref(cw), _stream()),
              'lirec_heads_loss_fwd_bwd_weighted')
    return loss, d_ints, d_rels, sel_out, probs


def _clip_weights(clip_weight, norm, clip_loss, B, dev):
    """The lirec_clip_weights of a loss call, or None when the call carries neither weights nor a per-clip output."""
    if clip_weight is None and clip_loss is None:
        return None
    cw = ClipWeights()
    if clip_weight is not None:
        assert clip_weight.device == dev and clip_weight.dtype in (torch.float32, torch.float64) and \
            clip_weight.numel() == B and clip_weight.is_contiguous()
        cw.w, cw.w_f64 = _p(clip_weight), int(clip_weight.dtype == torch.float64)
    if norm not in CLIP_WEIGHT_NORMS:
        raise LirecError("clip_weight_norm must be 'sum' or 'count', not %r" % (norm,))
    cw.norm = CLIP_WEIGHT_NORMS[norm]
    if clip_loss is not None:
        assert clip_loss.device == dev and clip_loss.dtype == torch.float32 and clip_loss.numel() == 2 * B and clip_loss.is_contiguous()
        cw.clip_loss = _p(clip_loss)
    return cw


def _set_divisors(a, divisors, dev):
    a.batch_divisor = a.rels_divisor = 0.0
    a.divisors_dev = None
    if divisors is None:
        return
    if torch.is_tensor(divisors):
        assert divisors.device == dev and divisors.dtype == torch.float32 and divisors.numel() >= 2 and divisors.is_contiguous()
        a.divisors_dev = _p(divisors)
    else:
        a.batch_divisor, a.rels_divisor = float(divisors[0]), float(divisors[1])


def ce_loss(ints, rels, y, r, class_w, B, Cc, NR, divisors=None, clip_weight=None, clip_weight_norm='sum', clip_loss=None):
    """``clip_weight`` / ``clip_weight_norm`` / ``clip_loss``: as margin_loss (the clip weight multiplies the class weight; the
    per-clip values are (cw[y_b] * CE_b, CE_b of the relationship row)).  ``divisors``: (sum of the targets' class weights, labelled relationship rows) of the GLOBAL batch, each divided by world (the
    data-parallel form, lirec_ce_loss); a pair of numbers or a device float32[2] tensor; None: this batch's own."""
    dev = ints.device
    d_ints = new((B, Cc), dtype=torch.float32, device=dev)
    d_rels = new((B, NR), dtype=torch.float32, device=dev) if rels is not None else None
    loss = new(1, dtype=torch.float32, device=dev)
    partial = new(2 * B + 2, dtype=torch.float32, device=dev)
    cw = _clip_weights(clip_weight, clip_weight_norm, clip_loss, B, dev)
    head = (_p(ints), ints.stride(0), _p(rels), rels.stride(0) if rels is not None else 0, _p(y), _p(r), _p(class_w), B, Cc, NR,
            _p(d_ints), Cc, _p(d_rels), NR, _p(loss), _p(partial), *_ce_divisors(divisors, dev))
    if cw is None:
        check(lib().lirec_ce_loss(*head, _stream()), 'lirec_ce_loss')
    else:
        check(lib().lirec_ce_loss_weighted(*head, C.byref(cw), _stream()), 'lirec_ce_loss_weighted')
    return loss, d_ints, d_rels


def adam_step_counted(p, g, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, count_dev, ticket, advance=True):
    """lirec_adam_step_counted: the step is ``count_dev`` (device int64[1], COMPLETED steps) + 1; ``advance``: the launch stores it back"""
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n and count_dev.dtype == torch.int64 and ticket.dtype == torch.int32
    check(lib().lirec_adam_step_counted(_p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, weight_decay, grad_scale,
                                        _p(count_dev), _p(ticket), int(bool(advance)), _stream()), 'lirec_adam_step_counted')


def _ce_divisors(divisors, dev):
    if divisors is None:
        return 0.0, 0.0, None
    if torch.is_tensor(divisors):
        assert divisors.device == dev and divisors.dtype == torch.float32 and divisors.numel() >= 2 and divisors.is_contiguous()
        return 0.0, 0.0, _p(divisors)
    return float(divisors[0]), float(divisors[1]), None


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, step_dev=None):
    """``step_dev``: optional device int64[1] tensor holding the 1-based step (read by the kernel instead of ``step``)."""
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    check(lib().lirec_adam_step(_p(p), _p(g), _p(m), _p(v), n, int(step), lr, beta1, beta2, eps, weight_decay,
                                grad_scale, _p(step_dev), _stream()), 'lirec_adam_step')


def _range_array(ranges, grouped=False):
    """the ctypes table of a range call: AdamRange (``grouped``: AdamGroupRange) entries from ``ranges`` = (offset, length, lag) /
    (offset, length, lag, group) tuples; a missing lag is 0.  An empty list gives one unused entry (the C side is handed a count)."""
    from ._lib import AdamRange, AdamGroupRange
    arr = ((AdamGroupRange if grouped else AdamRange) * max(len(ranges), 1))()
    for a, r in zip(arr, ranges):
        a.offset, a.length, a.lag = int(r[0]), int(r[1]), int(r[2]) if len(r) > 2 else 0
        if grouped:
            a.group = int(r[3])
    return arr


def adam_step_ranges(p, g, m, v, ranges, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, step_dev=None,
                     count_dev=None, ticket=None, advance=True):
    """lirec_adam_step_ranges: one launch over ``ranges`` = [(offset, length, lag), ...] (at most 64, ascending, offsets
    multiples of 4) of the flat buffers p, g, m, v given WHOLE (or from one common 16-byte-aligned base); range r is updated
    with step t - lag, t = ``step``, ``step_dev`` or ``count_dev`` + 1 (then ``ticket`` / ``advance`` as in adam_step_counted)."""
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    assert all(0 <= o and 0 <= k and o + k <= n for o, k, _ in ranges), 'a range outside the buffers'
    check(lib().lirec_adam_step_ranges(_p(p), _p(g), _p(m), _p(v), _range_array(ranges), len(ranges), int(step), lr, beta1, beta2, eps, weight_decay,
                                       grad_scale, _p(step_dev), _p(count_dev), _p(ticket), int(bool(advance)), _stream()),
          'lirec_adam_step_ranges')


def adam_hyper_write(table, rows):
    """lirec_adam_hyper_write: ``table`` (device float32, 8 words a row, 16-byte aligned) takes ``rows`` =
    [(lr, beta1, beta2, eps, weight_decay[, decoupled]), ...] (1..8; a row of five is a coupled one), by one tiny launch on the
    current stream -- the stream that reads it"""
    from ._lib import AdamHyper
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() >= 8 * len(rows)
    arr = (AdamHyper * max(len(rows), 1))()
    for a, row in zip(arr, rows):
        lr, b1, b2, eps, wd = row[:5]
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(lr), float(b1), float(b2), float(eps), float(wd)
        a.decoupled = 1.0 if len(row) > 5 and row[5] else 0.0
    check(lib().lirec_adam_hyper_write(_p(table), arr, len(rows), _stream()), 'lirec_adam_hyper_write')


def adam_step_groups(p, g, m, v, ranges, table, n_groups, step, grad_scale=1.0, step_dev=None, count_dev=None, ticket=None,
                     advance=True):
    """lirec_adam_step_groups: adam_step_ranges over ``ranges`` = [(offset, length, lag, group), ...] with the hyper-parameters
    of a range read from row ``group`` of the device ``table`` (adam_hyper_write) of ``n_groups`` rows"""
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    assert all(0 <= o and 0 <= k and o + k <= n for o, k, _, _ in ranges), 'a range outside the buffers'
    assert table.dtype == torch.float32 and table.numel() >= 8 * n_groups
    check(lib().lirec_adam_step_groups(_p(p), _p(g), _p(m), _p(v), _range_array(ranges, grouped=True), len(ranges), _p(table), int(n_groups), int(step),
                                       float(grad_scale), _p(step_dev), _p(count_dev), _p(ticket), int(bool(advance)), _stream()),
          'lirec_adam_step_groups')


class adam_hyper_row:
    """``with ops.adam_hyper_row(row):`` -- a folded first-layer update this host thread issues inside reads its hyper-parameters
    from the device row ``row`` (8 float32 words of a table; lirec_set_adam_hyper_row); cleared on the way out.  ``None``: nothing
    is set."""

    def __init__(self, row):
        self.row = row

    def __enter__(self):
        if self.row is not None:
            assert self.row.dtype == torch.float32
            check(lib().lirec_set_adam_hyper_row(_p(self.row)), 'lirec_set_adam_hyper_row')
        return self

    def __exit__(self, *exc):
        if self.row is not None:
            check(lib().lirec_set_adam_hyper_row(None), 'lirec_set_adam_hyper_row')
        return False


class adam_hyper_map:
    """``with ops.adam_hyper_map(table, ranges):`` -- a folded first-layer update this host thread issues inside takes ONE ROW PER
    PARAMETER: ``ranges`` = [(offset, length, group), ...] of the flat layout (at most 16), ``table`` the device table the groups
    index (lirec_set_adam_hyper_map); cleared on the way out.  ``table`` None: nothing is set."""

    def __init__(self, table, ranges=()):
        self.table, self.ranges = table, list(ranges)

    def __enter__(self):
        if self.table is not None:
            assert self.table.dtype == torch.float32
            arr = _range_array([(o, k, 0, grp) for o, k, grp in self.ranges], grouped=True)
            check(lib().lirec_set_adam_hyper_map(_p(self.table), arr, len(self.ranges)), 'lirec_set_adam_hyper_map')
        return self

    def __exit__(self, *exc):
        if self.table is not None:
            check(lib().lirec_set_adam_hyper_map(None, None, 0), 'lirec_set_adam_hyper_map')
        return False


def grad_sq_partials(g, ranges, partials):
    """lirec_grad_sq_partials: ``partials`` (device float64[CLIP_PARTIALS]) = the fixed grid's sums of squares of ``g`` over
    ``ranges`` = [(offset, length), ...] (1..64, offsets multiples of 4; a third entry -- a lag -- is ignored)"""
    from ._lib import CLIP_PARTIALS
    assert partials.dtype == torch.float64 and partials.numel() >= CLIP_PARTIALS and partials.is_contiguous()
    assert all(0 <= r[0] and 0 <= r[1] and r[0] + r[1] <= g.numel() for r in ranges), 'a range outside the buffer'
    check(lib().lirec_grad_sq_partials(_p(_f32c(g)), _range_array([r[:2] for r in ranges]), len(ranges), _p(partials), _stream()), 'lirec_grad_sq_partials')


def param_stats_ws_bytes(n_ranges):
    """lirec_param_stats_ws_bytes: the bytes of workspace a ``param_stats`` call over ``n_ranges`` entries needs"""
    return int(lib().lirec_param_stats_ws_bytes(int(n_ranges)))


def param_stats(p, g, m, v, entries, out, ws):
    """lirec_param_stats: row r of ``out`` (device float64[len(entries), 9], contiguous) = (sum of squares over the finite values,
    largest finite magnitude, count of non-finite values) of the gradient ``g``, of the parameter ``p`` and of the update direction
    (m inv_bc1) / (sqrt(v) inv_sqrt_bc2 + eps) over elements [offset, offset + length) of the flat fp32 buffers -- ``entries`` =
    [(offset, length, flags[, inv_bc1, inv_sqrt_bc2, eps]), ...] (1..64, any offsets), ``flags``: 1 gradient | 2 parameter | 4 update;
    a group not asked for is 0, and a buffer no entry asks for may be None.  ``ws``: device scratch of at least
    ``param_stats_ws_bytes(len(entries))`` bytes.  Two launches on the current stream; the same bits every time."""
    from ._lib import PARAM_STATS_COLS, ParamStatEntry
    n = len(entries)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= PARAM_STATS_COLS * n
    assert ws.is_contiguous()
    arr = (ParamStatEntry * max(n, 1))()
    for a, e in zip(arr, entries):
        a.offset, a.length, a.flags = int(e[0]), int(e[1]), int(e[2])
        a.inv_bc1, a.inv_sqrt_bc2, a.eps = (float(e[3]), float(e[4]), float(e[5])) if len(e) > 3 else (1.0, 1.0, 0.0)
        for bit, bufs in ((1, (g,)), (2, (p,)), (4, (m, v))):
            if a.flags & bit:
                assert all(b is not None and a.offset + a.length <= b.numel() for b in bufs), 'a range outside the buffers it asks for'
    bufs = [None if b is None else _p(_f32c(b)) for b in (p, g, m, v)]
    check(lib().lirec_param_stats(*bufs, arr, n, _p(out), _p(ws), ws.numel() * ws.element_size(), _stream()), 'lirec_param_stats')


def clip_finalize(partials, sq, mode, grad_scale, max_norm, out):
    """lirec_clip_finalize: ``sq`` (device float64[1]) = / += the sum of ``partials`` (mode 0 / 1; 2: as it stands), then
    ``out`` (device float32[2]) = (clip coefficient, norm = sqrt(sq) * grad_scale)"""
    assert sq.dtype == torch.float64 and out.dtype == torch.float32 and out.numel() >= 2 and out.is_contiguous()
    assert partials is None or partials.dtype == torch.float64
    check(lib().lirec_clip_finalize(_p(partials), _p(sq), int(mode), float(grad_scale), float(max_norm), _p(out), _stream()),
          'lirec_clip_finalize')


class adam_clip:
    """``with ops.adam_clip(coef):`` -- the Adam launches this host thread issues inside multiply their gradients by the device
    float ``coef`` (lirec_set_adam_clip); cleared on the way out, also when a launch raises.  ``None``: nothing is set."""

    def __init__(self, coef):
        self.coef = coef

    def __enter__(self):
        if self.coef is not None:
            assert self.coef.dtype == torch.float32
            check(lib().lirec_set_adam_clip(_p(self.coef)), 'lirec_set_adam_clip')
        return self

    def __exit__(self, *exc):
        if self.coef is not None:
            check(lib().lirec_set_adam_clip(None), 'lirec_set_adam_clip')
        return False


def clip_finalize_guard(partials, sq, mode, grad_scale, max_norm, out, skipped=None, count=False):
    """lirec_clip_finalize_guard: clip_finalize (``max_norm`` 0: coefficient 1) that also writes ``out[2]`` = 1.0 when ``sq`` is not
    finite, else 0 (``out``: device float32[>= 3]), and -- ``count`` -- adds that to ``skipped`` (device int64[1])"""
    assert sq.dtype == torch.float64 and out.dtype == torch.float32 and out.numel() >= 3 and out.is_contiguous()
    assert partials is None or partials.dtype == torch.float64
    assert skipped is None or skipped.dtype == torch.int64
    check(lib().lirec_clip_finalize_guard(_p(partials), _p(sq), int(mode), float(grad_scale), float(max_norm), _p(out), _p(skipped),
                                          int(bool(count)), _stream()), 'lirec_clip_finalize_guard')


class adam_guard:
    """``with ops.adam_guard(out, skipped):`` -- the Adam launches this host thread issues inside are the guarded ones: no-ops
    when the device float ``out[2]`` is set, otherwise scaled by ``out[0]`` with the step less the device int64 ``skipped``
    (lirec_set_adam_guard); cleared on the way out, also when a launch raises.  ``out`` None: nothing is set."""

    def __init__(self, out, skipped=None):
        self.out, self.skipped = out, skipped

    def __enter__(self):
        if self.out is not None:
            assert self.out.dtype == torch.float32 and self.out.numel() >= 3 and self.skipped.dtype == torch.int64
            check(lib().lirec_set_adam_guard(_p(self.out), _p(self.skipped)), 'lirec_set_adam_guard')
        return self

    def __exit__(self, *exc):
        if self.out is not None:
            check(lib().lirec_set_adam_guard(None, None), 'lirec_set_adam_guard')
        return False


def accum_scale(grad_scale, k):
    """the fp32 scale an update applies to the SUM of a window of ``k`` micro-batch gradients: (float)((double)(float)grad_scale
    / k), what the launches under ``adam_hold`` compute from their ``grad_scale`` -- the eager apply step passes it by value"""
    return C.c_float(C.c_float(float(grad_scale)).value / int(k)).value


class adam_hold:
    """``with ops.adam_hold(hold, k):`` -- the Adam and EMA launches this host thread issues inside read the device int64
    ``hold`` (word 1 of an accumulation window block, written by ``accum_begin``) and do nothing while it is set; otherwise they
    scale their gradients by ``accum_scale(grad_scale, k)`` (lirec_set_adam_hold); cleared on the way out, also when a launch
    raises.  ``hold`` None: nothing is set."""

    def __init__(self, hold, k=0):
        self.hold, self.k = hold, int(k)

    def __enter__(self):
        if self.hold is not None:
            assert self.hold.dtype == torch.int64 and self.k >= 1
            check(lib().lirec_set_adam_hold(_p(self.hold), self.k), 'lirec_set_adam_hold')
        return self

    def __exit__(self, *exc):
        if self.hold is not None:
            check(lib().lirec_set_adam_hold(None, 0), 'lirec_set_adam_hold')
        return False


def accum_begin(t, ctr, every, apply, win, k):
    """lirec_accum_begin, the head launch of a micro-step under gradient accumulation: zero the contiguous device tensor ``t``
    when the micro-step opens a window, ``ctr[i] += every[i]`` always and ``+= apply[i]`` when it closes one, the hold flag and
    the phase of the window block ``win`` (device int64[4], 16-byte aligned) advanced -- one launch."""
    assert t.is_contiguous() and ctr.dtype == torch.int64 and len(every) == len(apply) <= 4 and ctr.numel() >= len(every)
    assert win.dtype == torch.int64 and win.numel() >= 4 and win.is_contiguous()
    n = len(every)
    ev = (C.c_int64 * max(n, 1))(*[int(i) for i in every])
    ap = (C.c_int64 * max(n, 1))(*[int(i) for i in apply])
    check(lib().lirec_accum_begin(_p(t), t.numel() * t.element_size(), _p(ctr) if n else None, ev, ap, n, _p(win), int(k), _stream()),
          'lirec_accum_begin')


def ema_weight(decay):
    """the fp32 weight of one EMA update: the rounding of the double 1.0 - decay, as torch casts the Python scalar of
    ``lerp(ema, p, 1 - decay)``; ``decay`` outside (0.5, 1) -- NaN included -- is a ValueError (torch's lerp takes another
    branch from weight 0.5 on, which lirec_ema_step does not implement)"""
    d = float(decay)
    if not 0.5 < d < 1.0:
        raise ValueError('ema_decay must satisfy 0.5 < decay < 1, not %r' % (decay,))
    w = C.c_float(1.0 - d).value
    if not 0.0 < w < 0.5:
        raise ValueError('ema_decay %r leaves no fp32 weight in (0, 0.5)' % (decay,))
    return w


def ema_step(ema, p, weight, guard=None):
    """lirec_ema_step: ``ema`` <- fmaf(weight, p - ema, ema) elementwise (torch's ``ema.lerp_(p, weight)``, weight < 0.5, bit
    for bit), one launch on the current stream; ``ema`` and ``p``: contiguous fp32 device tensors of one length, at the same
    offset modulo 16 bytes.  ``guard``: the ``out`` block of clip_finalize_guard -- the launch does nothing when ``guard[2]`` is set."""
    n = ema.numel()
    assert p.numel() == n and ema.is_contiguous() and p.is_contiguous() and ema.dtype == torch.float32 and p.dtype == torch.float32
    assert guard is None or (guard.dtype == torch.float32 and guard.numel() >= 3 and guard.is_contiguous())
    check(lib().lirec_ema_step(_p(ema), _p(p), n, float(weight), _p(guard), _stream()), 'lirec_ema_step')


def counter_add(ctr, incs):
    """ctr[i] += incs[i] on the device (ctr: int64 device tensor, len(incs) <= 4)."""
    assert ctr.dtype == torch.int64 and ctr.is_cuda and 1 <= len(incs) <= 4 and ctr.numel() >= len(incs)
    arr = (C.c_int64 * len(incs))(*[int(i) for i in incs])
    check(lib().lirec_counter_add(_p(ctr), arr, len(incs), _stream()), 'lirec_counter_add')


def zero_count(t, ctr=None, incs=()):
    """Zero the contiguous device tensor ``t`` and add ``incs`` to the int64 device counters ``ctr`` in one launch."""
    assert t.is_contiguous() and (ctr is None or (ctr.dtype == torch.int64 and ctr.numel() >= len(incs)))
    arr = (C.c_int64 * max(len(incs), 1))(*[int(i) for i in incs])
    check(lib().lirec_zero_count(_p(t), t.numel() * t.element_size(), _p(ctr) if len(incs) else None, arr, len(incs), _stream()),
          'lirec_zero_count')


SNAPSHOT_MAX_RANGES = 8


def snapshot(pairs, digests):
    """lirec_snapshot: every ``(src, dst)`` of ``pairs`` (1 .. 8 pairs of contiguous device tensors of equal byte size, a multiple
    of 4, on 16-byte boundaries; no ``dst`` sharing a byte with any ``src`` or other ``dst``) copied bit for bit by ONE launch on
    the current stream, which leaves in ``digests[i]`` (int64 device tensor, at least ``len(pairs)`` words, zeroed by the call) the
    sum of pair i's 32-bit words modulo 2^64 (as a signed word: ``digests.view(torch.uint64)`` / numpy ``.view('u8')`` to compare)."""
    n = len(pairs)
    assert digests.dtype == torch.int64 and digests.is_contiguous() and digests.numel() >= n
    for s, d in pairs:
        assert s.is_contiguous() and d.is_contiguous() and s.numel() * s.element_size() == d.numel() * d.element_size()
    # (an empty view answers data_ptr() with 0: its place in its storage is what the call is given)
    at = lambda t: t.data_ptr() or (t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())
    src = (C.c_void_p * max(n, 1))(*[at(s) for s, _ in pairs])
    dst = (C.c_void_p * max(n, 1))(*[at(d) for _, d in pairs])
    nbytes = (C.c_int64 * max(n, 1))(*[s.numel() * s.element_size() for s, _ in pairs])
    check(lib().lirec_snapshot(src, dst, nbytes, n, _p(digests), _stream()), 'lirec_snapshot')


def cast_f64_f32(src, dst=None):
    assert src.dtype == torch.float64 and src.is_contiguous()
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    check(lib().lirec_cast_f64_f32(_p(src), _p(dst), src.numel(), _stream()), 'lirec_cast_f64_f32')
    return dst


def gather_features(clip, track, index, out_dtype=torch.float32):
    """(B, T, R+1, D) fp32 feature block from the de-duplicated piece tables (lirec_gather_features): row =
    [clip[index[...,0]] | track[index[...,1]] | track[index[...,2]]], zeros for a negative index."""
    assert clip.is_cuda and track.is_cuda and index.is_cuda and index.dtype == torch.int32 and index.shape[-1] == 3
    assert clip.dtype == track.dtype and clip.dtype in (torch.float32, torch.float64)
    assert out_dtype in (torch.float32, torch.bfloat16)       # bfloat16: "bf16 feature storage", rounded to nearest even
    clip, track, index = clip.contiguous(), track.contiguous(), index.contiguous()
    cd, td = clip.shape[1], track.shape[1]
    rows = index.numel() // 3
    out = torch.empty(tuple(index.shape[:-1]) + (cd + 2 * td,), dtype=out_dtype, device=index.device)
    fn = lib().lirec_gather_features if out_dtype == torch.float32 else lib().lirec_gather_features_bf16
    check(fn(_p(clip), cd, _p(track), td, int(clip.dtype == torch.float64), _p(index), rows, cd, td,
             _p(out), cd + 2 * td, _stream()), 'lirec_gather_features')
    return out


def dropout_mask(rows, cols, seed, p, site, device):
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    d = make_dropout(seed, p)
    check(lib().lirec_dropout_mask(_p(keep), rows, cols, C.byref(d), site, _stream()), 'lirec_dropout_mask')
    return keep


def set_gemm_mode(mode: int):
    check(lib().lirec_set_gemm_mode(mode), 'lirec_set_gemm_mode')


def get_gemm_mode() -> int:
    """the GEMM core of the current library context"""
    return int(lib().lirec_get_gemm_mode())


def set_grad_overwrite(on: bool):
    """weight / bias gradients overwrite their buffers instead of accumulating (lirec_set_grad_overwrite)"""
    check(lib().lirec_set_grad_overwrite(int(bool(on))), 'lirec_set_grad_overwrite')


def grad_overwrite_conflicts() -> int:
    """gradient buffers written by more than one launch since the overwrite mode was last switched on (this thread)"""
    return int(lib().lirec_grad_overwrite_conflicts())


def library_calls() -> int:
    """Number of library calls made by this process so far."""
    from . import _lib
    return _lib._calls[0]


def profile_enable(on: bool):
    check(lib().lirec_profile_enable(int(on)), 'lirec_profile_enable')


def profile_read() -> dict:
    """site name -> dict(ms, launches, flops, bytes) accumulated since profile_enable(True)."""
    L = lib()
    out = {}
    for s in range(L.lirec_profile_sites()):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(L.lirec_profile_read(s, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), 'lirec_profile_read')
        if n.value:
            out[L.lirec_profile_site_name(s).decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
    return out


_scratch = {}          # context handle (0 = default context) -> registered split-K scratch tensor


def _ctx_key():
    h = lib().lirec_ctx_get_current()
    return int(h) if h else 0


def ensure_scratch(device, nbytes: int = 256 << 20):
    """Register (once per library context) the split-K scratch buffer with the library."""
    key = _ctx_key()
    t = _scratch.get(key)
    if t is None or t.device != torch.device(device) or t.numel() * 4 < nbytes:
        t = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        check(lib().lirec_set_scratch(_p(t), t.numel() * 4), 'lirec_set_scratch')
        _scratch[key] = t
    return t


def release_scratch():
    check(lib().lirec_set_scratch(None, 0), 'lirec_set_scratch')
    _scratch.pop(_ctx_key(), None)


class Context:
    """A library context (include/lirec_hip.h, "Contexts"): its own GEMM core selection, split-K scratch and diagnostic
    switches.  Calls made inside ``with ctx:`` on this thread use it; everything else uses the default context.  Give
    each concurrently used stream its own context (e.g. evaluation on a side stream while training runs)."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().lirec_ctx_create(C.byref(h)), 'lirec_ctx_create')
        self.handle, self._prev = h, None

    def __enter__(self):
        self._prev = lib().lirec_ctx_get_current()
        check(lib().lirec_ctx_set_current(self.handle), 'lirec_ctx_set_current')
        return self

    def __exit__(self, *exc):
        check(lib().lirec_ctx_set_current(self._prev), 'lirec_ctx_set_current')
        return False

    def close(self):
        if self.handle is not None:
            _scratch.pop(int(self.handle.value or 0), None)
            check(lib().lirec_ctx_destroy(self.handle), 'lirec_ctx_destroy')
            self.handle = None


EVAL_COUNTERS = ('total', 'total_cl', 'total_rels', '_top1', '_trks_top1', '_cls_top1', '_rels_top1')


def eval_max_tracks(ints, rels, mem, y, r, g, just_zeros, counters, B, T, Cc, NR, loader_types=False):
    """Adds one batch to the device-side evaluation counters (int64[8], order EVAL_COUNTERS);
    utils/evaluation.py:114-176 (rels None) / :179-271."""
    assert counters.dtype == torch.int64 and counters.numel() >= 8 and counters.is_cuda
    fdt, idt = (torch.float64, torch.int64) if loader_types else (torch.float32, torch.int32)
    assert (mem is None or mem.dtype == fdt) and y.dtype == idt and g.dtype == idt and (r is None or r.dtype == idt)
    assert just_zeros is None or just_zeros.dtype in (torch.bool, torch.uint8)
    a = EvalArgs()
    a.ints, a.ld_ints = _p(_f32c(ints)), ints.stride(0)
    a.rels, a.ld_rels = _p(rels), (rels.stride(0) if rels is not None else 0)
    a.mem, a.y, a.r, a.g, a.just_zeros, a.counters = _p(mem), _p(y), _p(r), _p(g), _p(just_zeros), _p(counters)
    a.B, a.T, a.C, a.NR = B, T, Cc, NR
    a.loader_types = int(bool(loader_types))
    check(lib().lirec_eval_max_tracks(C.byref(a), _stream()), 'lirec_eval_max_tracks')


EVAL_TOPK_COUNTERS = ('total', '_top1', '_top3', '_top5', '_top1_sf', '_top5_sf')


def eval_clip_topk(logits, y, counters, conf=None, soft=None, y_stride=1, loader_types=False):
    """Adds one batch to the device-side clip-level counters (int64[8], order EVAL_TOPK_COUNTERS) and, with ``conf``, to the
    int64 [C, C] confusion matrix; Precision.update_probs, utils/evaluation.py:68-107, with the order of
    ``np.argsort(-x, kind='stable')`` (include/lirec_hip.h).  ``logits``: fp32 [B, C], the rows may be a strided view
    (``inters.reshape(bs, -1, C)[:, 0]``).  ``y``: 1-D, the label of clip b is ``y[b * y_stride]`` (the tensor's own stride
    counts too).  ``soft``: [B, n_soft], padded with -1.  ``loader_types``: y int64 and soft float64, else int32 / float32."""
    assert counters.dtype == torch.int64 and counters.numel() >= 8 and counters.is_cuda and counters.is_contiguous()
    assert logits.dim() == 2, tuple(logits.shape)
    B, Cc = logits.shape
    fdt, idt = (torch.float64, torch.int64) if loader_types else (torch.float32, torch.int32)
    assert y.dtype == idt and y.dim() == 1 and y_stride >= 1 and (B == 0 or y.numel() > (B - 1) * y_stride), (y.dtype, tuple(y.shape))
    assert conf is None or (conf.dtype == torch.int64 and tuple(conf.shape) == (Cc, Cc) and conf.is_contiguous())
    assert soft is None or (soft.dtype == fdt and soft.dim() == 2 and soft.shape[0] == B and soft.stride(1) == 1), 'soft labels'
    if B == 0:                # (an empty tensor has no address to hand over; the library's answer to B == 0 is "no launch" too)
        return
    a = EvalTopkArgs()
    # (a dimension of one element may carry any stride: the row stride only matters from the second row on)
    a.logits, a.ld_logits = _p(_f32c(logits)), (logits.stride(0) if B > 1 else Cc)
    a.y, a.y_stride = _p(y), (y.stride(0) * y_stride if y.numel() > 1 else 1)
    if soft is not None:
        a.soft, a.ld_soft, a.n_soft = _p(soft), (soft.stride(0) if B > 1 else soft.shape[1]), soft.shape[1]
    a.counters, a.conf = _p(counters), _p(conf)
    a.B, a.C = B, Cc
    a.loader_types = int(bool(loader_types))
    check(lib().lirec_eval_clip_topk(C.byref(a), _stream()), 'lirec_eval_clip_topk')


PREDICT_FIELDS = ('trk', 'cls', 'rel', 'score', 'trk_score', 'top_cls', 'top_cls_p', 'top_rel', 'top_rel_p', 'flags')


def predict_buffers(n, T, K, device, with_rels=True):
    """The output arrays of ``predict_clips`` for ``n`` clips of ``T`` tracks (include/lirec_hip.h: lirec_predict_args), on
    ``device``; ``top_rel`` / ``top_rel_p`` only ``with_rels``."""
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)
    out = {'trk': i32(n), 'cls': i32(n), 'rel': i32(n), 'score': torch.empty(n, dtype=torch.float64, device=device),
           'trk_score': torch.empty(n, T, dtype=torch.float64, device=device), 'top_cls': i32(n, K),
           'top_cls_p': torch.empty(n, K, dtype=torch.float32, device=device), 'flags': i32(n)}
    if with_rels:
        out['top_rel'], out['top_rel_p'] = i32(n, K), torch.empty(n, K, dtype=torch.float32, device=device)
    return out


def predict_clips(ints, rels=None, mem=None, B=None, T=1, K=5, loader_types=False, out=None):
    """Per-clip predictions without labels (lirec_predict_clips, include/lirec_hip.h): the joint (track, class[, relationship])
    argmax of the evaluation kernels, its score, the per-track scores and the top-``K`` lists of the predicted track.
    ``ints``: fp32 [B*T, C] and ``rels``: fp32 [B*T, NR] or None -- the rows may be strided views; ``mem``: [B, T] 0/1 fp32
    (``loader_types``: float64) or None; ``T = 1`` with ``mem = None`` is the clip-level form.  ``out``: a dict of contiguous
    device arrays for ``B`` clips to write into (any subset of ``PREDICT_FIELDS`` that holds ``trk``; e.g. slices of
    ``predict_buffers`` for a whole dataset) -- None: allocated here, on the logits' device.  Returns the dict."""
    assert ints.dim() == 2, tuple(ints.shape)
    rows, Cc = ints.shape
    B = rows // T if B is None else B
    assert B * T == rows and 1 <= K <= _lib.PREDICT_MAX_K, (B, T, rows, K)
    assert rels is None or (rels.dim() == 2 and rels.shape[0] == rows), 'rels'
    assert mem is None or (mem.dtype == (torch.float64 if loader_types else torch.float32) and mem.numel() == rows
                           and mem.is_contiguous()), 'mem'
    NR = rels.shape[1] if rels is not None else 0
    if out is None:
        out = predict_buffers(B, T, K, ints.device, with_rels=rels is not None)
    shapes = {'trk': (B,), 'cls': (B,), 'rel': (B,), 'score': (B,), 'trk_score': (B, T), 'top_cls': (B, K), 'top_cls_p': (B, K),
              'top_rel': (B, K), 'top_rel_p': (B, K), 'flags': (B,)}
    dtypes = {'score': torch.float64, 'trk_score': torch.float64, 'top_cls_p': torch.float32, 'top_rel_p': torch.float32}
    assert 'trk' in out, 'predict_clips: the output dict must hold trk'
    for k, t in out.items():
        assert tuple(t.shape) == shapes[k] and t.dtype == dtypes.get(k, torch.int32) and t.is_contiguous(), (k, tuple(t.shape), t.dtype)
    if B == 0:                # (an empty tensor has no address to hand over; the library's answer to B == 0 is "no launch" too)
        return out
    a = PredictArgs()
    # (a dimension of one element may carry any stride: the row stride only matters from the second row on)
    a.ints, a.ld_ints = _p(_f32c(ints)), (ints.stride(0) if rows > 1 else Cc)
    if rels is not None:
        a.rels, a.ld_rels = _p(_f32c(rels)), (rels.stride(0) if rows > 1 else NR)
    a.mem = _p(mem)
    for k, t in out.items():
        if k in ('top_rel', 'top_rel_p') and rels is None:
            continue
        setattr(a, k, _p(t))
    a.B, a.T, a.C, a.NR, a.K = B, T, Cc, NR, K
    a.loader_types = int(bool(loader_types))
    check(lib().lirec_predict_clips(C.byref(a), _stream()), 'lirec_predict_clips')
    return out


def _cursor_word(cursor):
    assert cursor.dtype == torch.int64 and cursor.is_cuda and cursor.numel() >= 1, 'cursor: an int64 device word'
    return _p(cursor)


def predict_clips_at(ints, rels, mem, cursor, out, B=None, T=1, K=5, loader_types=False):
    """``predict_clips`` into rows ``[cursor[0], cursor[0] + B)`` of DATASET-SIZED arrays (lirec_predict_clips_at): ``out`` -- a dict
    of ``predict_buffers`` arrays, all of one row count n -- is written at the row an int64 device word names when the kernel runs,
    so the launch, replayed from a command list, writes the next batch's rows once ``counter_add(cursor, [B])`` has moved the
    word.  The cursor is not moved here; trusted: 0 <= cursor[0] <= n - B.  Inputs as ``predict_clips``.  Returns ``out``."""
    assert ints.dim() == 2, tuple(ints.shape)
    rows, Cc = ints.shape
    B = rows // T if B is None else B
    assert B >= 1 and B * T == rows and 1 <= K <= _lib.PREDICT_MAX_K, (B, T, rows, K)
    assert rels is None or (rels.dim() == 2 and rels.shape[0] == rows), 'rels'
    assert mem is None or (mem.dtype == (torch.float64 if loader_types else torch.float32) and mem.numel() == rows
                           and mem.is_contiguous()), 'mem'
    NR = rels.shape[1] if rels is not None else 0
    assert 'trk' in out, 'predict_clips_at: the output dict must hold trk'
    n = out['trk'].shape[0]
    assert n >= B, (n, B)
    tails = {'trk': (), 'cls': (), 'rel': (), 'score': (), 'trk_score': (T,), 'top_cls': (K,), 'top_cls_p': (K,), 'top_rel': (K,),
             'top_rel_p': (K,), 'flags': ()}
    dtypes = {'score': torch.float64, 'trk_score': torch.float64, 'top_cls_p': torch.float32, 'top_rel_p': torch.float32}
    a = PredictArgs()
    for k, t in out.items():
        assert tuple(t.shape) == (n,) + tails[k] and t.dtype == dtypes.get(k, torch.int32) and t.is_contiguous(), (k, tuple(t.shape), t.dtype)
        if k in ('top_rel', 'top_rel_p') and rels is None:
            continue
        setattr(a, k, _p(t))
    # (a dimension of one element may carry any stride: the row stride only matters from the second row on)
    a.ints, a.ld_ints = _p(_f32c(ints)), (ints.stride(0) if rows > 1 else Cc)
    if rels is not None:
        a.rels, a.ld_rels = _p(_f32c(rels)), (rels.stride(0) if rows > 1 else NR)
    a.mem = _p(mem)
    a.B, a.T, a.C, a.NR, a.K = B, T, Cc, NR, K
    a.loader_types = int(bool(loader_types))
    check(lib().lirec_predict_clips_at(C.byref(a), _cursor_word(cursor), _stream()), 'lirec_predict_clips_at')
    return out


def rows_copy_at(src, dst, cursor):
    """``dst[cursor[0]:cursor[0] + rows] = src`` for fp32 matrices, the row read from an int64 device word when the kernel runs
    (lirec_rows_copy_at): ``src`` [rows, cols], possibly a strided view of unit column stride, ``dst`` [n, cols] with n >= rows.  The
    cursor is not moved; trusted: 0 <= cursor[0] <= n - rows."""
    assert src.dim() == 2 and dst.dim() == 2 and src.shape[1] == dst.shape[1] >= 1 and dst.shape[0] >= src.shape[0], (tuple(src.shape), tuple(dst.shape))
    rows, cols = src.shape
    if rows == 0:
        return
    _f32c(src), _f32c(dst)
    check(lib().lirec_rows_copy_at(_p(src), src.stride(0) if rows > 1 else cols, rows, cols, _p(dst),
                                   dst.stride(0) if dst.shape[0] > 1 else cols, _cursor_word(cursor), _stream()), 'lirec_rows_copy_at')


def scalar_accumulate(acc, v):
    """``acc[0] += v[0]`` on the device (lirec_scalar_accumulate): ``acc`` a one-element fp32 or float64 device tensor, ``v`` fp32 --
    bit for bit torch's ``acc += v``, as a launch a command list can carry."""
    assert acc.numel() >= 1 and acc.dtype in (torch.float32, torch.float64) and v.numel() >= 1 and v.dtype == torch.float32, (acc.dtype, v.dtype)
    check(lib().lirec_scalar_accumulate(_p(acc), int(acc.dtype == torch.float64), _p(v), _stream()), 'lirec_scalar_accumulate')


def collate_fields(ids, fields):
    """dst row b = src row ids[b] for every (src [N, ...], dst [B, ...]) pair of contiguous device tensors, byte for byte, in one
    launch on the current stream (lirec_collate_fields).  ``ids``: int32 [B], trusted (the caller validated them)."""
    B = ids.numel()
    assert ids.dtype == torch.int32 and ids.is_contiguous() and len(fields) <= _lib.COLLATE_MAX_FIELDS, len(fields)
    if B == 0 or not fields:
        return
    arr = (_lib.CollateField * len(fields))()
    for f, (src, dst) in enumerate(fields):
        rb = src[0].numel() * src.element_size()
        assert src.is_contiguous() and dst.is_contiguous() and dst.numel() * dst.element_size() == B * rb, (f, tuple(src.shape), tuple(dst.shape))
        arr[f].src, arr[f].row_bytes, arr[f].dst = _p(src), rb, _p(dst)
    check(lib().lirec_collate_fields(_p(ids), B, arr, len(fields), _stream()), 'lirec_collate_fields')


def collate_fields_at(ids_base, cursor, B, fields):
    """``collate_fields`` for the ``B`` ids at ``ids_base[cursor[0]:]`` -- ``cursor``: an int64 device word the kernel reads when it
    runs, so the launch, replayed from a command list, draws the batch the cursor names then (lirec_collate_fields_at).  The cursor
    is not moved (``counter_add(cursor, [B])`` behind the call does that); trusted: 0 <= cursor[0] <= ids_base.numel() - B."""
    assert ids_base.dtype == torch.int32 and ids_base.is_contiguous() and ids_base.is_cuda and ids_base.numel() >= B >= 1, B
    assert cursor.dtype == torch.int64 and cursor.is_cuda and cursor.numel() >= 1 and len(fields) <= _lib.COLLATE_MAX_FIELDS, len(fields)
    if not fields:
        return
    arr = (_lib.CollateField * len(fields))()
    for f, (src, dst) in enumerate(fields):
        rb = src[0].numel() * src.element_size()
        assert src.is_contiguous() and dst.is_contiguous() and dst.numel() * dst.element_size() == B * rb, (f, tuple(src.shape), tuple(dst.shape))
        arr[f].src, arr[f].row_bytes, arr[f].dst = _p(src), rb, _p(dst)
    check(lib().lirec_collate_fields_at(_p(ids_base), _p(cursor), B, arr, len(fields), _stream()), 'lirec_collate_fields_at')


def collate_workspace(n_clip_all, n_track_all, device):
    """A workspace for ``collate_resident`` over stores of these row counts (uint8; the library clears it in every call)."""
    need = int(lib().lirec_collate_workspace_bytes(int(n_clip_all), int(n_track_all)))
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


def collate_resident(ids, index_rows, n_clip_all, n_track_all, feature_index, clip_rows, track_rows, counts, fields, workspace):
    """One batch buffer of a resident-store dataset written on the device (lirec_collate_resident, include/lirec_hip.h): what
    ``features.collate(store=, static_layout=True)`` + ``batch_to_device`` put there.  ``ids``: int32 [B] sample ids (trusted: the
    caller validated them); ``index_rows``: int32 [N, E, 3] (or [N, T, R + 1, 3]) stacked sample table; ``feature_index`` int32
    [B, E, 3], ``clip_rows`` / ``track_rows`` int32 row lists of the static layout's lengths, ``counts`` int32 [2]: written.
    ``fields``: (src [N, ...], dst [B, ...]) pairs of contiguous tensors, rows copied byte for byte.  ``workspace``:
    ``collate_workspace``.  Everything on the current stream; nothing is read back."""
    B = ids.numel()
    N = index_rows.shape[0]
    E = index_rows.numel() // (3 * N) if N else 0
    i32 = lambda t: t.dtype == torch.int32 and t.is_contiguous()
    assert i32(ids) and i32(index_rows) and i32(feature_index) and i32(clip_rows) and i32(track_rows) and i32(counts), 'int32, contiguous'
    assert index_rows.shape[-1] == 3 and feature_index.numel() == B * E * 3 and counts.numel() >= 2, (tuple(index_rows.shape), B, E)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
    assert len(fields) <= _lib.COLLATE_MAX_FIELDS, len(fields)
    if B == 0:                # (an empty tensor has no address to hand over; the library's answer to B == 0 is "no launch" too)
        return
    a = _lib.CollateArgs()
    a.ids, a.index_rows, a.feature_index = _p(ids), _p(index_rows), _p(feature_index)
    a.clip_rows, a.track_rows, a.counts = _p(clip_rows), _p(track_rows), _p(counts)
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    a.n_clip_all, a.n_track_all, a.n_clip_list, a.n_track_list = int(n_clip_all), int(n_track_all), clip_rows.numel(), track_rows.numel()
    a.B, a.E, a.nf = B, E, len(fields)
    for f, (src, dst) in enumerate(fields):
        rb = src[0].numel() * src.element_size()
        assert src.is_contiguous() and dst.is_contiguous() and src.shape[0] == N and dst.numel() * dst.element_size() == B * rb, \
            (f, tuple(src.shape), tuple(dst.shape))
        a.fields[f].src, a.fields[f].row_bytes, a.fields[f].dst = _p(src), rb, _p(dst)
    check(lib().lirec_collate_resident(C.byref(a), _stream()), 'lirec_collate_resident')


def draw_context(slot_dst, slot_off, pool_rows, index_rows, R, seed, epoch):
    """The epoch's draw from every over-long context list, IN PLACE in the resident ``index_rows`` (int32 [N, T, R + 1, 3] or
    [N, E, 3]) -- one launch on the current stream (lirec_draw_context, include/lirec_hip.h; ``features.draw_context`` is the rule in
    numpy).  ``slot_dst`` int32 [S], ``slot_off`` int32 [S + 1], ``pool_rows`` int32 [P, 3]: trusted (``PiecesDataset.device_tables``
    validated them).  ``seed``: 64 bits, ``epoch``: taken modulo 2^32, both by value."""
    S, N = slot_dst.numel(), index_rows.shape[0]
    i32 = lambda t: t.dtype == torch.int32 and t.is_contiguous()
    assert i32(slot_dst) and i32(slot_off) and i32(pool_rows) and i32(index_rows), 'int32, contiguous'
    assert slot_off.numel() == S + 1 and pool_rows.shape[-1] == 3 and index_rows.shape[-1] == 3, (S, tuple(slot_off.shape), tuple(pool_rows.shape))
    if S == 0:                # (an empty tensor has no address to hand over; the library's answer to S == 0 is "no launch" too)
        return
    a = _lib.DrawContextArgs()
    a.slot_dst, a.slot_off, a.pool_rows, a.index_rows = _p(slot_dst), _p(slot_off), _p(pool_rows), _p(index_rows)
    a.seed, a.epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF
    a.S, a.R, a.E = S, int(R), index_rows.numel() // (3 * N)
    check(lib().lirec_draw_context(C.byref(a), _stream()), 'lirec_draw_context')
