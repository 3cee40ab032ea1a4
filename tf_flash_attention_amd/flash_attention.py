"""Drop-in mirror of the reference's ``flash_attention/flash_attention.py`` on MI355X.

Public API (same names, argument meaning, defaults and return convention as
``/root/reference/flash_attention/flash_attention.py:80-370``)::

    full_1d(Q, K, V, sync_mode='none_front', returning_l_m=False)
    causal_1d(Q, K, V, sync_mode, returning_l_m=False)
    local_1d(Q, K, V, window_size, log2_stride_size, is_causal, sync_mode, returning_l_m=False)
    full_2d / causal_2d / local_2d   (same, for 2-D sequences)

Beyond the reference: attention of one ``Q`` over the union of several key sets, each under its own
rule (a window plus global tokens, self-attention plus a prompt, key shards), with exact gradients::

    combined_1d(Q, [Part('local', K, V, window_size=256), Part('full', Kg, Vg)], returning_l_m=False)
    combined_2d(Q, parts, returning_l_m=False)
    merge_partials(Os, ls, ms, seq_dims=1) -> (O, l, m)      (op level, no autograd)

and grouped-query attention (GQA / MQA), where ``Hq = g * Hk`` query heads share the K/V heads (the last
batch axis; query head ``h`` attends K/V head ``h // g``), with gradients::

    grouped_1d(Q, K, V, policy='full', sync_mode='none_front', window_size=1, log2_stride_size=0,
               is_causal=False, returning_l_m=False)
    grouped_2d(...)
    attention_forward_grouped(policy, seq_dims, Q, K, V, sync_mode, ...) -> (O, l, m)   (op level)

and decode over a padded K/V cache, where sequence ``s`` attends its first ``k_lens[s]`` keys and the lengths
are an int32 tensor on the device that the kernels read (no host synchronisation; inference only)::

    ragged_1d(Q, K, V, k_lens, tail_causal=False, returning_l_m=False)

or over a paged cache: pools ``[num_pages, Hk, C, page]`` of fixed-size pages and an int32 block table on the device
that says which page holds which keys of which sequence (also read by the kernels only)::

    paged_1d(Q, K_pool, V_pool, block_table, k_lens, tail_causal=False, returning_l_m=False)

Tensors are ``torch`` tensors on a ROCm device in the reference's channel-first
layout ``batch_shape + (C, *seq_shape)``.  Each call returns ``O`` or
``(O, l, m)``; autograd flows through ``O`` only (gradients of ``l``/``m`` are
ignored, as in ``flash_attention.py:382-384``).

``_fa_kernel`` exposes the op-level entry points under the snake_case names
TF generates for the reference's registered ops
(``flash_attention_forward.cc:144-253``, ``flash_attention_backward.cc:51-154``),
e.g. ``_fa_kernel.full_attention_forward1d_float16(q, k, v, sync_mode=...)`` and
``_fa_kernel.local_attention_backward2d(q, k, v, o, l, m, d_o, sync_mode=...,
window_size=..., log2_stride_size=..., is_causal=...)``.  They validate shapes
with the reference's exact messages (``flash_attention_forward.cc:97-140``,
``flash_attention_backward.cc:197-258``) and call the C ABI (``include/fa_api.h``)
on the current HIP stream.  There is no CPU / eager fallback.
"""

from __future__ import annotations

import ctypes
import re
from types import SimpleNamespace

import torch

from . import _lib

__all__ = [
    "full_1d", "causal_1d", "local_1d", "full_2d", "causal_2d", "local_2d",
    "InvalidArgumentError", "InternalError", "estimate_forward_flops",
    "Part", "combined_1d", "combined_2d", "merge_partials",
    "grouped_1d", "grouped_2d", "attention_forward_grouped",
    "ragged_1d", "paged_1d", "ragged_prefill_1d", "paged_prefill_1d", "quantize_kv_fp8",
    "ragged_append_1d", "paged_append_1d", "ragged_window_prefill_1d", "paged_window_prefill_1d",
]


class InvalidArgumentError(ValueError):
    """Mirror of tf.errors.InvalidArgumentError raised by the reference op kernels."""


class InternalError(RuntimeError):
    """Mirror of tf.errors.InternalError (kernel launch failures)."""


_DTYPES = {torch.float16: _lib.F16, torch.float32: _lib.F32, torch.float64: _lib.F64}
_POLICIES = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}


def _shape_str(shape) -> str:
    # TensorShape::DebugString() format
    return "[" + ",".join(str(int(s)) for s in shape) + "]"


def _sync_mode_id(sync_mode) -> int:
    if isinstance(sync_mode, bytes):
        sync_mode = sync_mode.decode()
    sid = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT,
           "scale_end": _lib.SCALE_END}.get(sync_mode, -1)
    if sid < 0:
        # FlashAttentionForwardBase ctor, flash_attention_forward.cc:274-276
        raise InvalidArgumentError(f"Unsupported sync_mode: {sync_mode}")
    return sid


def verify_and_extract_shapes(seq_dims, Q_shape, K_shape, V_shape):
    """VerifyAndExtractShapes<SequenceDims> (flash_attention_forward.cc:97-140)."""
    Q_shape, K_shape, V_shape = tuple(Q_shape), tuple(K_shape), tuple(V_shape)
    if not (len(Q_shape) == len(K_shape) == len(V_shape)):
        raise InvalidArgumentError("The number of dimensions of Q, K, and V should be equal")
    if len(Q_shape) < seq_dims + 2:
        raise InvalidArgumentError(f"The number of dimensions of Q, K, and V should be >= {seq_dims + 2}")
    ch = len(Q_shape) - seq_dims - 1
    Q_ch, K_ch, V_ch = Q_shape[ch], K_shape[ch], V_shape[ch]
    Qb, Qs = Q_shape[:ch], Q_shape[ch + 1:]
    Kb, Ks = K_shape[:ch], K_shape[ch + 1:]
    Vb, Vs = V_shape[:ch], V_shape[ch + 1:]
    if Q_ch != K_ch:
        raise InvalidArgumentError("The channel dimension of Q and K should be equal")
    if Qb != Kb or Qb != Vb:
        raise InvalidArgumentError(
            "The batch shape of all inputs should be equal, but Q_batch_shape = " + _shape_str(Qb)
            + ", K_batch_shape = " + _shape_str(Kb) + ", V_batch_shape = " + _shape_str(Vb) + " were received")
    if Ks != Vs:
        raise InvalidArgumentError(
            "The sequence shape of K and V are expected to be equal, but K_seq_shape = " + _shape_str(Ks)
            + ", V_seq_shape = " + _shape_str(Vs) + " are detected")
    return Qb, Qs, Q_ch, Kb, Ks, K_ch, Vb, Vs, V_ch


def verify_backward_shapes(seq_dims, Q, K, V, O, l, m, dO):
    """Checks of FlashAttentionBackwardBase::Compute (flash_attention_backward.cc:197-258)."""
    shapes = [tuple(t.shape) for t in (Q, K, V, O, l, m, dO)]
    Qs_, Ks_, Vs_, Os_, ls_, ms_, dOs_ = shapes
    if not (len(Qs_) == len(Ks_) == len(Vs_) == len(Os_) == len(dOs_)):
        raise InvalidArgumentError("The number of dimensions of Q, K, V, O, and dO should be equal")
    if not (len(ls_) == len(ms_) == len(Qs_) - 1):
        raise InvalidArgumentError("The number of dimensions of l and m should be equal to the one of Q minus 1")
    if len(Qs_) < seq_dims + 2:
        raise InvalidArgumentError(f"The number of dimensions of Q, K, V, O, and dO should be >= {seq_dims + 2}")
    ch = len(Qs_) - seq_dims - 1
    Q_ch, K_ch, V_ch, O_ch = Qs_[ch], Ks_[ch], Vs_[ch], Os_[ch]

    def split(s, lm=False):
        return s[:ch], (s[ch:] if lm else s[ch + 1:])

    (Qb, Qq), (Kb, Kk), (Vb, Vk), (Ob, Oq) = split(Qs_), split(Ks_), split(Vs_), split(Os_)
    (lb, lq), (mb, mq), (dOb, dOq) = split(ls_, True), split(ms_, True), split(dOs_)
    if Q_ch != K_ch:
        raise InvalidArgumentError("The channel dimension of Q and K should be equal")
    if V_ch != O_ch:
        raise InvalidArgumentError("The channel dimension of V and O should be equal")
    if not (Qb == Kb == Vb == Ob == lb == mb == dOb):
        raise InvalidArgumentError(
            "The batch shape of all inputs should be equal, but Q_batch_shape = " + _shape_str(Qb)
            + ", K_batch_shape = " + _shape_str(Kb) + ", V_batch_shape = " + _shape_str(Vb)
            + ", O_batch_shape = " + _shape_str(Ob) + ", l_batch_shape = " + _shape_str(lb)
            + ", m_batch_shape = " + _shape_str(mb) + ", dO_batch_shape = " + _shape_str(dOb) + " are received")
    if Kk != Vk:
        raise InvalidArgumentError(
            "The sequence shape of K and V should be equal, but K_seq_shape = " + _shape_str(Kk)
            + ", V_seq_shape = " + _shape_str(Vk) + " were received")
    if not (Qq == Oq == lq == mq == dOq):
        raise InvalidArgumentError(
            "The sequence shape of Q, O, l, m, and dO should be equal, but Q_seq_shape = " + _shape_str(Qq)
            + ", O_seq_shape = " + _shape_str(Oq) + ", l_seq_shape = " + _shape_str(lq)
            + ", m_seq_shape = " + _shape_str(mq) + ", dO_seq_shape = " + _shape_str(dOq) + " were received")
    return Qb, Qq, Q_ch, Kk, V_ch


def _prod(xs) -> int:
    n = 1
    for x in xs:
        n *= int(x)
    return n


def _check_device_tensors(*ts):
    dev = ts[0].device
    if dev.type != "cuda":
        raise InvalidArgumentError("flash attention tensors must live on a ROCm (cuda) device; there is no CPU kernel")
    for t in ts:
        if t.device != dev:
            raise InvalidArgumentError("all inputs must be on the same device")


def _dtype_id(t: torch.Tensor, float16_op: bool) -> int:
    dt = _DTYPES.get(t.dtype)
    if dt is None:
        raise TypeError(f"unsupported dtype {t.dtype}; expected float16, float32 or float64")
    if float16_op != (dt == _lib.F16):
        raise TypeError(f"op {'...Float16' if float16_op else '{float,double}'} does not accept {t.dtype}")
    return dt


def _raise_status(st: int, what: str):
    msg = _lib.last_error()
    if st == _lib.FA_ERR_INVALID_ARGUMENT:
        raise InvalidArgumentError(msg)
    if st == _lib.FA_ERR_UNSUPPORTED:
        raise InvalidArgumentError(msg)
    raise InternalError(msg or f"Failed to launch the {what} kernel ({st})")


def _stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def attention_forward(policy: str, seq_dims: int, Q, K, V, sync_mode, window_size=1, log2_stride_size=0,
                      is_causal=False, float16_op=None):
    """Op-level forward: returns (O, l, m).  Mirrors FlashAttentionForwardBase::Compute."""
    sid = _sync_mode_id(sync_mode)
    Qb, Qs, Q_ch, _, Ks, _, _, _, V_ch = verify_and_extract_shapes(seq_dims, Q.shape, K.shape, V.shape)
    if float16_op is None:
        float16_op = Q.dtype == torch.float16
    dt = _dtype_id(Q, float16_op)
    if K.dtype != Q.dtype or V.dtype != Q.dtype:
        raise TypeError("Q, K and V must share one dtype")
    _check_device_tensors(Q, K, V)
    Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
    l_dtype = torch.float32 if dt == _lib.F16 else Q.dtype
    O = torch.empty(Qb + (V_ch,) + Qs, dtype=Q.dtype, device=Q.device)
    l = torch.empty(Qb + Qs, dtype=l_dtype, device=Q.device)
    m = torch.empty(Qb + Qs, dtype=Q.dtype, device=Q.device)
    prob = _lib.make_problem(dt, _POLICIES[policy], seq_dims, sid, _prod(Qb), Qs, Ks, Q_ch, V_ch,
                             window_size, log2_stride_size, is_causal)
    L = _lib.lib()
    # few queries against a long key range: the split-key path needs scratch for its partials
    ws_bytes = int(L.fa_forward_workspace_bytes(prob))
    with torch.cuda.device(Q.device):
        if ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Q.device)
            st = L.fa_forward_ws(_stream_handle(Q.device), prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                 O.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
        else:
            st = L.fa_forward(_stream_handle(Q.device), prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                              O.data_ptr(), l.data_ptr(), m.data_ptr())
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    return O, l, m


def attention_backward(policy: str, seq_dims: int, Q, K, V, O, l, m, dO, sync_mode, window_size=1,
                       log2_stride_size=0, is_causal=False, float16_op=None):
    """Op-level backward: returns (dQ, dK, dV).  Mirrors FlashAttentionBackwardBase::Compute."""
    sid = _sync_mode_id(sync_mode)
    Qb, Qs, Q_ch, Ks, V_ch = verify_backward_shapes(seq_dims, Q, K, V, O, l, m, dO)
    if float16_op is None:
        float16_op = Q.dtype == torch.float16
    dt = _dtype_id(Q, float16_op)
    # the typed op inputs of flash_attention_backward.cc:51-154: q, k, v, o, m: T; l: float for the
    # Float16 ops, T otherwise (a mismatched l would be read at the wrong width)
    for name, t in (("K", K), ("V", V), ("O", O), ("m", m)):
        if t.dtype != Q.dtype:
            raise TypeError(f"{name} must have Q's dtype {Q.dtype}, got {t.dtype}")
    l_dtype = torch.float32 if dt == _lib.F16 else Q.dtype
    if l.dtype != l_dtype:
        raise TypeError(f"l must be {l_dtype} for this op, got {l.dtype}")
    _check_device_tensors(Q, K, V, O, l, m, dO)
    Q, K, V, O, l, m, dO = (t.contiguous() for t in (Q, K, V, O, l, m, dO))
    dO = dO.to(Q.dtype)
    dQ = torch.empty_like(Q)
    dK = torch.empty_like(K)
    dV = torch.empty_like(V)
    prob = _lib.make_problem(dt, _POLICIES[policy], seq_dims, sid, _prod(Qb), Qs, Ks, Q_ch, V_ch,
                             window_size, log2_stride_size, is_causal)
    L = _lib.lib()
    # few queries against a long key range: the dQ pass splits over key chunks; many queries against
    # one key block: the dK/dV pass splits over query chunks (more scratch either way); everywhere
    # else this is fa_backward and its workspace
    ws_bytes = L.fa_backward_split_workspace_bytes(prob)
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=Q.device)
    with torch.cuda.device(Q.device):
        st = L.fa_backward_split(_stream_handle(Q.device), prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                 O.data_ptr(), l.data_ptr(), m.data_ptr(), dO.data_ptr(), dQ.data_ptr(),
                                 dK.data_ptr(), dV.data_ptr(), ws.data_ptr(), ws_bytes)
    if st != _lib.FA_OK:
        _raise_status(st, "Backward")
    return dQ, dK, dV


class _AttentionFn(torch.autograd.Function):
    """Forward op + its registered gradient (flash_attention.py:392-471)."""

    @staticmethod
    def forward(ctx, Q, K, V, policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal):
        O, l, m = attention_forward(policy, seq_dims, Q, K, V, sync_mode, window_size, log2_stride_size, is_causal)
        ctx.save_for_backward(Q, K, V, O, l, m)
        ctx.attrs = (policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal)
        ctx.mark_non_differentiable(l, m)
        return O, l, m

    @staticmethod
    def backward(ctx, dO, dl, dm):
        # only the gradient w.r.t. O is propagated (flash_attention.py:382-384)
        Q, K, V, O, l, m = ctx.saved_tensors
        policy, seq_dims, sync_mode, ws, ls, causal = ctx.attrs
        if dO is None:
            dO = torch.zeros_like(O)
        dQ, dK, dV = attention_backward(policy, seq_dims, Q, K, V, O, l, m, dO, sync_mode, ws, ls, causal)
        return dQ, dK, dV, None, None, None, None, None, None


def _attend(policy, seq_dims, Q, K, V, sync_mode, returning_l_m, window_size=1, log2_stride_size=0,
            is_causal=False):
    results = _AttentionFn.apply(Q, K, V, policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal)
    return results if returning_l_m else results[0]


def full_1d(Q, K, V, sync_mode="none_front", returning_l_m=False):
    """Full attention on 1d sequences (flash_attention.py:80-119)."""
    return _attend("full", 1, Q, K, V, sync_mode, returning_l_m)


def causal_1d(Q, K, V, sync_mode, returning_l_m=False):
    """Causal attention on 1d sequences (flash_attention.py:122-160)."""
    return _attend("causal", 1, Q, K, V, sync_mode, returning_l_m)


def local_1d(Q, K, V, window_size, log2_stride_size, is_causal, sync_mode, returning_l_m=False):
    """Local attention on 1d sequences (flash_attention.py:163-216)."""
    return _attend("local", 1, Q, K, V, sync_mode, returning_l_m, window_size, log2_stride_size, is_causal)


def full_2d(Q, K, V, sync_mode="none_front", returning_l_m=False):
    """Full attention on 2d sequences (flash_attention.py:219-263)."""
    return _attend("full", 2, Q, K, V, sync_mode, returning_l_m)


def causal_2d(Q, K, V, sync_mode, returning_l_m=False):
    """Causal attention on 2d sequences (flash_attention.py:266-309)."""
    return _attend("causal", 2, Q, K, V, sync_mode, returning_l_m)


def local_2d(Q, K, V, window_size, log2_stride_size, is_causal, sync_mode, returning_l_m=False):
    """Local attention on 2d sequences (flash_attention.py:312-370)."""
    return _attend("local", 2, Q, K, V, sync_mode, returning_l_m, window_size, log2_stride_size, is_causal)


# ----------------------------------------------------------------------------
# Combined attention: one Q over the union of several key sets, each under its own rule
# (include/fa_api.h, "Merging partial results")
# ----------------------------------------------------------------------------
MAX_PARTS = _lib.FA_MAX_PARTS


class Part:
    """One key set of a combined attention and the rule Q attends it under: ``policy`` in
    {"full", "causal", "local"} with the arguments of the wrapper of that name."""

    __slots__ = ("policy", "K", "V", "sync_mode", "window_size", "log2_stride_size", "is_causal")

    def __init__(self, policy, K, V, sync_mode="none_front", window_size=1, log2_stride_size=0, is_causal=False):
        if policy not in _POLICIES:
            raise InvalidArgumentError(f"Unsupported policy: {policy}")
        self.policy, self.K, self.V, self.sync_mode = policy, K, V, sync_mode
        self.window_size, self.log2_stride_size, self.is_causal = int(window_size), int(log2_stride_size), bool(is_causal)

    def attrs(self):
        return self.policy, self.sync_mode, self.window_size, self.log2_stride_size, self.is_causal

    def __repr__(self):
        return (f"Part({self.policy!r}, K{_shape_str(self.K.shape)}, V{_shape_str(self.V.shape)}, "
                f"sync_mode={self.sync_mode!r}, window_size={self.window_size}, "
                f"log2_stride_size={self.log2_stride_size}, is_causal={self.is_causal})")


def _check_part_count(n):
    if not 1 <= n <= MAX_PARTS:
        raise InvalidArgumentError(f"The number of parts should be in [1, {MAX_PARTS}], but {n} were received")


def _same_dtype_and_device(ts):
    """One dtype (TypeError) and one ROCm device (InvalidArgumentError) for all of ``ts``."""
    for t in ts:
        if t.dtype != ts[0].dtype:
            raise TypeError(f"all tensors must share one dtype, got {ts[0].dtype} and {t.dtype}")
    _check_device_tensors(*ts)


def merge_partials(Os, ls, ms, seq_dims=1):
    """Op-level merge (no autograd): the forward outputs ``(O_i, l_i, m_i)`` of one Q against several key
    sets become ``(O, l, m)`` of Q against their union (``fa_merge_partials``).  Every part must come from
    the same Q (scale 1/sqrt(d)); a key present in two parts counts twice.  Example: key shards under the
    full policy, ``merge_partials(*zip(*[attention_forward("full", 1, Q, Ks, Vs, "none_front") for Ks, Vs in
    shards]))`` equals ``full_1d`` over the concatenated keys."""
    Os, ls, ms = list(Os), list(ls), list(ms)
    if not (len(Os) == len(ls) == len(ms)):
        raise InvalidArgumentError("The numbers of O, l and m partials should be equal")
    _check_part_count(len(Os))
    O0 = Os[0]
    if O0.dim() < seq_dims + 1:
        raise InvalidArgumentError(f"The number of dimensions of O should be >= {seq_dims + 1}")
    ch = O0.dim() - seq_dims - 1
    lm_shape = tuple(O0.shape[:ch]) + tuple(O0.shape[ch + 1:])
    for O, l, m in zip(Os, ls, ms):
        if tuple(O.shape) != tuple(O0.shape):
            raise InvalidArgumentError("The shapes of all O partials should be equal, but " + _shape_str(O0.shape)
                                       + " and " + _shape_str(O.shape) + " were received")
        if tuple(l.shape) != lm_shape or tuple(m.shape) != lm_shape:
            raise InvalidArgumentError(
                "The shapes of l and m should be the one of O without its channel dimension, but O_shape = "
                + _shape_str(O.shape) + ", l_shape = " + _shape_str(l.shape) + ", m_shape = " + _shape_str(m.shape)
                + " were received")
    dt = _dtype_id(O0, O0.dtype == torch.float16)
    l_dtype = torch.float32 if dt == _lib.F16 else O0.dtype
    for O, l, m in zip(Os, ls, ms):
        if O.dtype != O0.dtype or m.dtype != O0.dtype:
            raise TypeError(f"all O and m partials must have dtype {O0.dtype}, got {O.dtype} and {m.dtype}")
        if l.dtype != l_dtype:
            raise TypeError(f"l must be {l_dtype} for this dtype, got {l.dtype}")
    _check_device_tensors(*Os, *ls, *ms)
    Os, ls, ms = ([t.contiguous() for t in ts] for ts in (Os, ls, ms))
    O, l, m = torch.empty_like(Os[0]), torch.empty_like(ls[0]), torch.empty_like(ms[0])
    nq = _prod(O0.shape[ch + 1:])
    with torch.cuda.device(O.device):
        st = _lib.lib().fa_merge_partials(
            _stream_handle(O.device), dt, _prod(O0.shape[:ch]), nq, int(O0.shape[ch]), len(Os),
            _lib.pointer_array([t.data_ptr() for t in Os]), _lib.pointer_array([t.data_ptr() for t in ls]),
            _lib.pointer_array([t.data_ptr() for t in ms]), O.data_ptr(), l.data_ptr(), m.data_ptr())
    if st != _lib.FA_OK:
        _raise_status(st, "merge")
    return O, l, m


def _accumulate_parts(ts):
    """T(sum of ``ts`` in order, accumulated in fp32 / fp64): ``fa_accumulate_parts``."""
    if len(ts) == 1:
        return ts[0]
    ts = [t.contiguous() for t in ts]
    out = torch.empty_like(ts[0])
    with torch.cuda.device(out.device):
        st = _lib.lib().fa_accumulate_parts(_stream_handle(out.device), _DTYPES[out.dtype], out.numel(), len(ts),
                                            _lib.pointer_array([t.data_ptr() for t in ts]), out.data_ptr())
    if st != _lib.FA_OK:
        _raise_status(st, "accumulate")
    return out


class _CombinedFn(torch.autograd.Function):
    """Forward of every part + merge; the backward calls each part's backward op with the MERGED (O, l, m):
    P = exp(s - m) / l is then the union's probability, so dK_i and dV_i are exact and dQ = sum_i dQ_i."""

    @staticmethod
    def forward(ctx, Q, seq_dims, attrs, *KV):
        Os, ls, ms = [], [], []
        for i, (policy, sync_mode, ws, ls_, causal) in enumerate(attrs):
            O, l, m = attention_forward(policy, seq_dims, Q, KV[2 * i], KV[2 * i + 1], sync_mode, ws, ls_, causal)
            Os.append(O); ls.append(l); ms.append(m)
        O, l, m = merge_partials(Os, ls, ms, seq_dims)
        ctx.save_for_backward(Q, *KV, O, l, m)  # (not the partials)
        ctx.attrs = (seq_dims, attrs)
        ctx.mark_non_differentiable(l, m)
        return O, l, m

    @staticmethod
    def backward(ctx, dO, dl, dm):
        Q, *KV, O, l, m = ctx.saved_tensors
        seq_dims, attrs = ctx.attrs
        if dO is None:
            dO = torch.zeros_like(O)
        need = ctx.needs_input_grad
        dQs, dKV = [], []
        for i, (policy, sync_mode, ws, ls_, causal) in enumerate(attrs):
            if not (need[0] or need[3 + 2 * i] or need[4 + 2 * i]):
                dKV += [None, None]
                continue
            # (a part whose K and V need no gradient still contributes its dQ)
            dQ, dK, dV = attention_backward(policy, seq_dims, Q, KV[2 * i], KV[2 * i + 1], O, l, m, dO, sync_mode,
                                            ws, ls_, causal)
            dQs.append(dQ)
            dKV += [dK, dV]
        return (_accumulate_parts(dQs) if need[0] else None, None, None, *dKV)


def _combined(seq_dims, Q, parts, returning_l_m):
    parts = list(parts)
    _check_part_count(len(parts))
    for p in parts:
        if not isinstance(p, Part):
            raise TypeError(f"parts must be Part records, got {type(p).__name__}")
        _sync_mode_id(p.sync_mode)
        verify_and_extract_shapes(seq_dims, Q.shape, p.K.shape, p.V.shape)
    ch = Q.dim() - seq_dims - 1
    for p in parts:
        if p.V.shape[ch] != parts[0].V.shape[ch]:
            raise InvalidArgumentError(
                "The channel dimension of V should be equal in all parts, but " + str(int(parts[0].V.shape[ch]))
                + " and " + str(int(p.V.shape[ch])) + " were received")
    KV = [t for p in parts for t in (p.K, p.V)]
    _dtype_id(Q, Q.dtype == torch.float16)
    _same_dtype_and_device([Q] + KV)
    results = _CombinedFn.apply(Q, seq_dims, tuple(p.attrs() for p in parts), *KV)
    return results if returning_l_m else results[0]


def combined_1d(Q, parts, returning_l_m=False):
    """Attention of Q over the union of the key sets of ``parts`` (1 to 8 :class:`Part` records), each under
    its own rule, on 1d sequences: softmax over all the parts' allowed keys at scale 1/sqrt(d).  Every part
    runs the forward it runs alone; the results are merged on the device.  Gradients flow to Q and to every
    part's K and V, exactly (through each part's normaliser too).  Returns ``O`` or ``(O, l, m)``."""
    return _combined(1, Q, parts, returning_l_m)


def combined_2d(Q, parts, returning_l_m=False):
    """:func:`combined_1d` for 2d sequences."""
    return _combined(2, Q, parts, returning_l_m)


# ----------------------------------------------------------------------------
# Grouped-query attention: g = Hq / Hk query heads share one K/V head
# (include/fa_api.h, "Grouped-query forward")
# ----------------------------------------------------------------------------
def verify_grouped_shapes(seq_dims, Q_shape, K_shape, V_shape):
    """The checks of verify_and_extract_shapes, with the batch shapes allowed to differ in their last axis
    (the heads): Q ``batch + (Hq, C, *Nq)``, K ``batch + (Hk, C, *Nk)``, V ``batch + (Hk, Cv, *Nk)``,
    Hq = g * Hk.  Returns (Q batch shape, Q seq shape, C, K/V batch shape, K seq shape, Cv, g)."""
    Q_shape, K_shape, V_shape = tuple(Q_shape), tuple(K_shape), tuple(V_shape)
    if not (len(Q_shape) == len(K_shape) == len(V_shape)):
        raise InvalidArgumentError("The number of dimensions of Q, K, and V should be equal")
    if len(Q_shape) < seq_dims + 2:
        raise InvalidArgumentError(f"The number of dimensions of Q, K, and V should be >= {seq_dims + 2}")
    ch = len(Q_shape) - seq_dims - 1
    Qb, Kb, Vb = Q_shape[:ch], K_shape[:ch], V_shape[:ch]
    Qs, Ks, Vs = Q_shape[ch + 1:], K_shape[ch + 1:], V_shape[ch + 1:]
    if Q_shape[ch] != K_shape[ch]:
        raise InvalidArgumentError("The channel dimension of Q and K should be equal")
    if Kb != Vb or Qb[:-1] != Kb[:-1]:
        raise InvalidArgumentError(
            "The batch shapes of K and V should be equal, and equal to the one of Q except in its last axis, "
            "but Q_batch_shape = " + _shape_str(Qb) + ", K_batch_shape = " + _shape_str(Kb) + ", V_batch_shape = "
            + _shape_str(Vb) + " were received")
    if Ks != Vs:
        raise InvalidArgumentError(
            "The sequence shape of K and V are expected to be equal, but K_seq_shape = " + _shape_str(Ks)
            + ", V_seq_shape = " + _shape_str(Vs) + " are detected")
    g = 1
    if ch > 0 and Qb[-1] != Kb[-1]:
        if Kb[-1] < 1 or Qb[-1] % Kb[-1] != 0:
            raise InvalidArgumentError(
                "The last batch axis of Q should be a multiple of the one of K and V, but Q_batch_shape = "
                + _shape_str(Qb) + ", K_batch_shape = " + _shape_str(Kb) + " were received")
        g = int(Qb[-1]) // int(Kb[-1])
    return Qb, Qs, Q_shape[ch], Kb, Ks, V_shape[ch], g


def _expand_groups(t, ch, g):
    """K or V with every head repeated g times along the last batch axis (repeat_interleave)."""
    return t if g == 1 else t.repeat_interleave(g, dim=ch - 1)


def attention_forward_grouped(policy: str, seq_dims: int, Q, K, V, sync_mode, window_size=1, log2_stride_size=0,
                              is_causal=False):
    """Op-level grouped forward: Q slice (..., h) attends K/V slice (..., h // g); returns (O, l, m) with Q's
    batch shape.  Inside the fused envelope (``fa_forward_grouped_plan`` reports chunks) K and V stream once
    per group; everywhere else K and V are expanded and ``attention_forward`` runs, so every dtype, rule,
    channel count and split plan works."""
    sid = _sync_mode_id(sync_mode)
    Qb, Qs, Q_ch, Kb, Ks, V_ch, g = verify_grouped_shapes(seq_dims, Q.shape, K.shape, V.shape)
    ch = len(Qb)
    if g == 1:
        return attention_forward(policy, seq_dims, Q, K, V, sync_mode, window_size, log2_stride_size, is_causal)
    dt = _dtype_id(Q, Q.dtype == torch.float16)
    if K.dtype != Q.dtype or V.dtype != Q.dtype:
        raise TypeError("Q, K and V must share one dtype")
    _check_device_tensors(Q, K, V)
    prob = _lib.make_problem(dt, _POLICIES[policy], seq_dims, sid, _prod(Qb), Qs, Ks, Q_ch, V_ch,
                             window_size, log2_stride_size, is_causal)
    L = _lib.lib()
    plan = (ctypes.c_int32 * 6)()
    st = L.fa_forward_grouped_plan(prob, g, plan)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    if plan[0] == 0:  # outside the fused envelope
        return attention_forward(policy, seq_dims, Q, _expand_groups(K, ch, g), _expand_groups(V, ch, g), sync_mode,
                                 window_size, log2_stride_size, is_causal)
    Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
    O = torch.empty(Qb + (V_ch,) + Qs, dtype=Q.dtype, device=Q.device)
    l = torch.empty(Qb + Qs, dtype=torch.float32, device=Q.device)
    m = torch.empty(Qb + Qs, dtype=Q.dtype, device=Q.device)
    ws_bytes = int(L.fa_forward_grouped_workspace_bytes(prob, g))
    with torch.cuda.device(Q.device):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=Q.device)
        st = L.fa_forward_grouped(_stream_handle(Q.device), prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                  O.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    return O, l, m


class _GroupedFn(torch.autograd.Function):
    """Grouped forward + its gradient.  The backward always runs the ungrouped backward op on expanded K and V
    with the saved (O, l, m) — also after a fused forward: the op reads only the tensors it is given — and
    sums dK and dV over each group in fp32 (fp64 for double) with one rounding.  (There is no grouped
    backward kernel: the fused envelope is decode, which has no backward.)"""

    @staticmethod
    def forward(ctx, Q, K, V, policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal):
        O, l, m = attention_forward_grouped(policy, seq_dims, Q, K, V, sync_mode, window_size, log2_stride_size,
                                            is_causal)
        ctx.save_for_backward(Q, K, V, O, l, m)
        ctx.attrs = (policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal)
        ctx.mark_non_differentiable(l, m)
        return O, l, m

    @staticmethod
    def backward(ctx, dO, dl, dm):
        Q, K, V, O, l, m = ctx.saved_tensors
        policy, seq_dims, sync_mode, ws, ls, causal = ctx.attrs
        if dO is None:
            dO = torch.zeros_like(O)
        ch = Q.dim() - seq_dims - 1
        g = int(Q.shape[ch - 1]) // int(K.shape[ch - 1])
        dQ, dKe, dVe = attention_backward(policy, seq_dims, Q, _expand_groups(K, ch, g), _expand_groups(V, ch, g),
                                          O, l, m, dO, sync_mode, ws, ls, causal)
        acc = torch.float64 if Q.dtype == torch.float64 else torch.float32

        def fold(t, like):  # [..., Hk * g, C, N...] -> sum over g
            s = tuple(like.shape)
            return t.reshape(s[:ch] + (g,) + s[ch:]).sum(dim=ch, dtype=acc).to(like.dtype)

        return dQ, fold(dKe, K), fold(dVe, V), None, None, None, None, None, None


def _grouped(seq_dims, Q, K, V, policy, sync_mode, window_size, log2_stride_size, is_causal, returning_l_m):
    if policy not in _POLICIES:
        raise InvalidArgumentError(f"Unsupported policy: {policy}")
    _sync_mode_id(sync_mode)
    *_, g = verify_grouped_shapes(seq_dims, Q.shape, K.shape, V.shape)
    if g == 1:  # bit for bit the ungrouped wrapper
        return _attend(policy, seq_dims, Q, K, V, sync_mode, returning_l_m, window_size, log2_stride_size, is_causal)
    results = _GroupedFn.apply(Q, K, V, policy, seq_dims, sync_mode, window_size, log2_stride_size, is_causal)
    return results if returning_l_m else results[0]


def grouped_1d(Q, K, V, policy="full", sync_mode="none_front", window_size=1, log2_stride_size=0, is_causal=False,
               returning_l_m=False):
    """Grouped-query attention on 1d sequences: Q ``batch + (Hq, C, Nq)``, K ``batch + (Hk, C, Nk)``, V ``batch +
    (Hk, Cv, Nk)`` with Hq = g * Hk read from the shapes; query head h attends K/V head h // g (the
    ``repeat_interleave`` convention), under ``policy`` in {"full", "causal", "local"} with the arguments of the
    wrapper of that name.  fp16 problems with g * next_pow2(Nq) <= 128 and at most 128 channels stream K and V
    once per group; every other problem runs on expanded K and V.  Gradients flow to Q, K and V; dK and dV are
    the sums over each group's heads.  Returns ``O`` or ``(O, l, m)``."""
    return _grouped(1, Q, K, V, policy, sync_mode, window_size, log2_stride_size, is_causal, returning_l_m)


def grouped_2d(Q, K, V, policy="full", sync_mode="none_front", window_size=1, log2_stride_size=0, is_causal=False,
               returning_l_m=False):
    """:func:`grouped_1d` for 2d sequences."""
    return _grouped(2, Q, K, V, policy, sync_mode, window_size, log2_stride_size, is_causal, returning_l_m)


# ----------------------------------------------------------------------------
# Ragged few-query forward: decode over a padded K/V cache with per-sequence key lengths on the device
# (include/fa_api.h, "Ragged few-query forward")
# ----------------------------------------------------------------------------
_RAGGED_ENVELOPE = ("float16, 1d sequences, at most 128 channels, Nq >= 1, capacity >= 1 and "
                    "g * next_pow2(Nq) <= 128 with g = Hq / Hk")


# An FP8 K/V cache (include/fa_api.h, "over an FP8 K/V cache"): OCP e4m3fn bytes, as
# torch.float8_e4m3fn or as the same bytes in a uint8 tensor
_FP8_CACHE_DTYPES = tuple(dt for dt in (getattr(torch, "float8_e4m3fn", None), torch.uint8) if dt is not None)
FP8_E4M3_MAX = 448.0


def quantize_kv_fp8(x, head_axis, scale=None):
    """Quantizes a K or V tensor to ``torch.float8_e4m3fn`` with one scale per K/V head: returns ``(x8, scale)``
    with ``x ~= scale[h] * x8`` along ``head_axis``.  Without ``scale`` it is the head's ``amax / 448`` over all
    other axes (1.0 for a head of zeros); a given ``scale`` is a float32 tensor of shape ``(Hk,)``.  ``x / scale`` is
    clamped to +-448 before the cast, because the cast itself turns what lies beyond the format's range into NaN.
    Plain torch, on the device of ``x``: appends are a few tokens per step, so this is not a kernel.  The fused
    appends ``ragged_append_1d`` / ``paged_append_1d`` store the same bytes for given scales, in the cache's own
    kernel."""
    if getattr(torch, "float8_e4m3fn", None) is None:
        raise NotImplementedError("this torch has no float8_e4m3fn")
    head_axis = head_axis % x.dim()
    xf = x.to(torch.float32)
    if scale is None:
        amax = xf.abs().amax(dim=[a for a in range(x.dim()) if a != head_axis])
        scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    elif not isinstance(scale, torch.Tensor) or scale.dtype != torch.float32:
        raise TypeError(f"scale must be a float32 tensor, got {getattr(scale, 'dtype', type(scale).__name__)}")
    elif tuple(scale.shape) != (x.shape[head_axis],):
        raise InvalidArgumentError("The shape of scale should be (Hk,) = " + _shape_str((x.shape[head_axis],))
                                   + ", but scale_shape = " + _shape_str(scale.shape) + " was received")
    view = [1] * x.dim()
    view[head_axis] = -1
    x8 = (xf / scale.to(xf.device).view(view)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return x8, scale


def _kv_cache_scales(what, Q, K, V, hk, k_scale, v_scale, q="Q"):
    """Whether K and V are an FP8 cache, after the checks of their dtypes and of the scales (fp32 device tensors of
    shape ``(Hk,)``, or None for 1.0).  ``q`` names the float16 tensor ``Q`` in the messages (an append has no Q)."""
    fp8 = K.dtype in _FP8_CACHE_DTYPES
    if fp8:
        if V.dtype not in _FP8_CACHE_DTYPES:
            raise TypeError(f"{what} must both be an FP8 cache (float8_e4m3fn or uint8) or both share the dtype of {q}")
    elif K.dtype != Q.dtype or V.dtype != Q.dtype:
        raise TypeError(f"{q}, {what} must share one dtype")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is None:
            continue
        if not fp8:
            raise InvalidArgumentError(f"{name} was given, but {what} are not an FP8 cache (float8_e4m3fn or uint8): "
                                       "a float16 cache takes no scale")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if tuple(t.shape) != (hk,):
            raise InvalidArgumentError(f"The shape of {name} should be (Hk,) = " + _shape_str((hk,)) + f", but {name}_shape = "
                                       + _shape_str(t.shape) + " was received")
        if t.device != Q.device:
            raise InvalidArgumentError(f"{name} must be on the device of {q}")
        if not t.is_contiguous():  # (the kernels read the caller's own array on every replay, not a copy)
            raise InvalidArgumentError(f"{name} must be contiguous")
    return fp8


def _scale_ptrs(fp8, k_scale, v_scale):
    """The (k_scale, v_scale) arguments that an FP8 forward takes after V (None: 1.0); none for a float16 cache."""
    return tuple(t.data_ptr() if t is not None else None for t in (k_scale, v_scale)) if fp8 else ()


# (cache, form, fp8) -> the names of the (plan, workspace_bytes, forward) entry points
decode_entry_points = _lib.decode_entry_points


def _decode_form(prefill, window, mask=None):
    """The form of a decode call: query-blocked (under a window or not), under a window (an int), tree-masked (a
    tensor), or plain."""
    if prefill and window is not None:
        return "window_prefill"
    return "prefill" if prefill else "tree" if mask is not None else "plain" if window is None else "window"


def _decode_window(what, window_size, tail_causal, nq):
    """The window of a windowed ``ragged_1d`` / ``paged_1d`` call as an int, or None without one."""
    if window_size is None:
        return None
    if isinstance(window_size, bool) or not isinstance(window_size, int):
        raise TypeError(f"window_size must be an int or None, got {type(window_size).__name__}")
    if window_size < 1:
        raise InvalidArgumentError(f"{what}: window_size must be >= 1, but window_size = {window_size} was received")
    if nq > 1 and not tail_causal:
        raise InvalidArgumentError(f"{what}: a window places the Nq = {nq} queries at the last Nq positions of the "
                                   "sequence, which is the tail rule, so window_size with Nq > 1 requires "
                                   "tail_causal=True")
    return min(window_size, 2 ** 31 - 1)  # (any window at or above the capacity is the tail rule)


def _decode_mask(what, draft_mask, tail_causal, window_size, Q, batch, nq):
    """The mask of a tree-masked ``ragged_1d`` / ``paged_1d`` call as a contiguous int32 tensor, or None without one."""
    if draft_mask is None:
        return None
    if not isinstance(draft_mask, torch.Tensor) or draft_mask.dtype != torch.int32:
        raise TypeError("draft_mask must be an int32 tensor or None, got "
                        f"{getattr(draft_mask, 'dtype', type(draft_mask).__name__)}")
    want = tuple(batch) + (nq, (nq + 31) // 32)
    if tuple(draft_mask.shape) != want:
        raise InvalidArgumentError("The shape of draft_mask should be the batch shape without the heads plus "
                                   "(Nq, ceil(Nq / 32)), but draft_mask_shape = " + _shape_str(draft_mask.shape)
                                   + ", expected " + _shape_str(want) + " were received")
    if draft_mask.device != Q.device:
        raise InvalidArgumentError("draft_mask must be on the device of Q")
    if not tail_causal:
        raise InvalidArgumentError(f"{what}: draft slot j is the key at position k_lens - Nq + j, which is the tail "
                                   "rule's placement, so draft_mask requires tail_causal=True")
    if window_size is not None:
        raise InvalidArgumentError(f"{what}: there is no windowed tree form; give draft_mask or window_size, not both")
    return draft_mask.contiguous()


def draft_mask_from_parents(parents):
    """The ``draft_mask`` of a forest of draft tokens: ``parents`` is an integer tensor ``batch + (Nq,)`` with
    ``parents[..., i] < i`` the parent of node i, or -1 for a child of the committed context.  Returns the int32
    tensor ``batch + (Nq, ceil(Nq / 32))`` in which node i sees itself and its ancestors, built on the device of
    ``parents`` without a host read: ancestors come before their descendants, so one pass in node order completes
    every row from its parent's."""
    if not isinstance(parents, torch.Tensor) or parents.dtype.is_floating_point or parents.dtype == torch.bool:
        raise TypeError(f"parents must be an integer tensor, got {getattr(parents, 'dtype', type(parents).__name__)}")
    if parents.dim() < 1 or parents.shape[-1] < 1:
        raise InvalidArgumentError("parents should be batch + (Nq,) with Nq >= 1, but parents_shape = "
                                   + _shape_str(parents.shape) + " was received")
    nq = int(parents.shape[-1])
    words = (nq + 31) // 32
    par = parents.to(torch.int64)
    sees = torch.zeros(tuple(parents.shape) + (32 * words,), dtype=torch.bool, device=parents.device)
    for i in range(nq):
        p = par[..., i]
        up = torch.gather(sees, -2, p.clamp(0, nq - 1)[..., None, None].expand(p.shape + (1, 32 * words)))[..., 0, :]
        sees[..., i, :] = up & ((p >= 0) & (p < i))[..., None]
        sees[..., i, i] = True
    weights = torch.ones(32, dtype=torch.int64, device=parents.device) << torch.arange(32, device=parents.device)
    packed = (sees.view(tuple(parents.shape) + (words, 32)).to(torch.int64) * weights).sum(-1)
    return (packed - ((packed >> 31) << 32)).to(torch.int32)  # (bit 31 is the int32's sign)


def ragged_1d(Q, K, V, k_lens, tail_causal=False, returning_l_m=False, k_scale=None, v_scale=None, window_size=None,
              draft_mask=None):
    """Attention of a few queries over a padded K/V cache: Q ``batch + (Hq, C, Nq)``, K ``batch + (Hk, C, cap)``,
    V ``batch + (Hk, Cv, cap)`` with Hq = g * Hk read from the shapes (query head h attends K/V head h // g), and
    ``k_lens`` an int32 tensor of shape ``batch`` on the same device (0-d without a leading batch axis): sequence
    s attends only its first ``k_lens[s]`` keys, clamped to [0, cap]; what K and V hold behind them is ignored.
    With ``tail_causal`` the Nq queries are the last Nq positions of the sequence: query i sees keys
    j <= k_lens[s] - Nq + i.  Rows that see no key get O = 0, l = 0 and m of bytes 0xFA.

    The lengths are read by the kernels, never on the host: no synchronisation, and a captured graph may be
    replayed after ``k_lens`` was overwritten in place.  Inference only (no gradient); float16 only; outside the
    fused envelope the call raises NotImplementedError (a fallback would have to read the lengths on the host).

    An FP8 cache: K and V of dtype ``torch.float8_e4m3fn`` (or the same bytes as ``torch.uint8``) with Q float16.
    ``k_scale`` and ``v_scale`` are float32 tensors of shape ``(Hk,)`` on the device of Q, or None for 1.0: the true
    key of head h is ``k_scale[h] * K[..., h, :, :]``, the true value ``v_scale[h] * V[..., h, :, :]``
    (``quantize_kv_fp8`` makes both).  The kernels read the scales, never the host.  A float16 cache takes no scale.

    A sliding window: ``window_size`` = W >= 1 (None: no window).  The queries sit at the last Nq positions of the
    sequence, so Nq > 1 requires ``tail_causal=True`` (for Nq = 1 either value is accepted): query i at position
    ``pos = k_lens[s] - Nq + i`` sees the W keys ``max(0, pos - W + 1) <= j <= pos``, its own position included
    (``local_1d``'s window with ``is_causal``).  The launched work, the workspace and the time follow W + Nq - 1,
    not the capacity; ``W >= cap`` is the tail-causal call itself, bit for bit.  With
    ``lo = max(0, k_lens[s] - Nq - W + 1)``, keys below ``lo // 64 * 64`` are never read.  The at most 63 keys
    between that and ``lo`` are read and masked, so they must be finite (they are the sequence's own earlier keys).

    A tree of draft tokens (speculative decoding that verifies several candidates in one step): ``draft_mask`` is an
    int32 tensor ``batch + (Nq, ceil(Nq / 32))`` on the device of Q, taken as raw bits and shared by all heads of a
    sequence.  The Nq queries are the draft tokens at the last Nq positions (``tail_causal=True`` is required, and
    ``window_size`` must be None): draft slot j is the key at ``base + j``, ``base = k_lens[s] - Nq``, and query i
    sees the keys below ``base`` and the slots j with bit ``j & 31`` of ``draft_mask[s, i, j >> 5]`` set; slots at
    negative positions name no key, and bits at or past Nq are ignored.  ``draft_mask_from_parents`` builds the mask
    of a forest (each token sees itself and its ancestors); the lower triangle is the ``tail_causal`` call, bit for
    bit.  The kernels read the mask, never the host, so it too may be overwritten in place between replays.  Draft
    keys that a query does not see are read and masked: they must be finite.

    More queries than the envelope's g * next_pow2(Nq) <= 128 (chunked prefill, a long speculative draft):
    ``ragged_prefill_1d``.  Returns ``O`` or ``(O, l, m)``."""
    return _ragged_forward("ragged_1d", False, Q, K, V, k_lens, tail_causal, returning_l_m, k_scale, v_scale, window_size,
                           draft_mask)


def ragged_prefill_1d(Q, K, V, k_lens, tail_causal=False, returning_l_m=False, k_scale=None, v_scale=None):
    """``ragged_1d`` for any number of queries (chunked prefill, long speculative drafts): the same tensors, layouts,
    ``tail_causal`` rule, empty rows, FP8 cache and scales, with Nq >= 1 unbounded and 1 <= g <= 128.  The queries are
    worked in blocks of P = the largest power of two with g * P <= 128; where one block holds them all the call is
    ``ragged_1d`` itself, bit for bit.  There is no ``window_size``.  (Under a sliding window:
    ``ragged_window_prefill_1d``.)

    A batch that mixes prefill with decode right-aligns each sequence's real queries in the Nq slots (with
    ``tail_causal`` the last slot is the sequence's last position).  The padding queries in front compute earlier
    positions' rows, or empty rows where they lie before position 0; the caller ignores them.

    ``k_lens`` and the scales are read by the kernels, never on the host.  Inference only; float16 only; outside
    the envelope (more than 128 channels, g > 128) the call raises NotImplementedError.  Returns ``O`` or
    ``(O, l, m)``."""
    return _ragged_forward("ragged_prefill_1d", True, Q, K, V, k_lens, tail_causal, returning_l_m, k_scale, v_scale, None)


def ragged_window_prefill_1d(Q, K, V, k_lens, window_size, returning_l_m=False, k_scale=None, v_scale=None):
    """``ragged_1d`` under a sliding window for any number of queries (chunked prefill of local-attention layers): the
    same tensors, layouts, empty rows, FP8 cache and scales, with Nq >= 1 unbounded and 1 <= g <= 128.
    ``window_size`` = W is a required int >= 1 (clamped to 2^31 - 1).  The Nq queries are the last Nq positions of the
    sequence (the tail rule is implied): query i at position ``pos = k_lens[s] - Nq + i`` sees the W keys
    ``max(0, pos - W + 1) <= j <= pos``; a query before position 0 gets the empty row.  The queries are worked in
    blocks of P = the largest power of two with g * P <= 128, and each block launches work for the W + P - 1 keys it
    can see, not for the prefix.  ``W >= cap`` is ``ragged_prefill_1d(..., tail_causal=True)`` itself and one block is
    ``ragged_1d(..., tail_causal=True, window_size=W)`` itself, bit for bit.

    ``k_lens`` and the scales are read on the device, never on the host: no synchronisation, and the call may be
    replayed from a captured graph after they were overwritten in place.  A batch that mixes prefill with decode
    right-aligns each sequence's real queries in the Nq slots; the padding queries in front compute earlier
    positions' rows, or empty rows.  With ``lo = max(0, k_lens[s] - Nq - W + 1)``, the call's lowest window start,
    keys below ``lo // 64 * 64`` are never read; the up to 63 keys between that and ``lo`` are read and masked, so
    they must be finite.  Attention sinks compose from a second call and ``merge_partials``, as in ``ragged_1d``.

    Inference only; float16 only; outside the envelope (more than 128 channels, g > 128) the call raises
    NotImplementedError.  Returns ``O`` or ``(O, l, m)``."""
    return _ragged_forward("ragged_window_prefill_1d", True, Q, K, V, k_lens, True, returning_l_m, k_scale, v_scale,
                           _required_window(window_size))


def _required_window(window_size):
    """``window_size`` of a call that has no form without one."""
    if window_size is None:
        raise TypeError("window_size must be an int, got None")
    return window_size


_PREFILL_ENVELOPE = ("float16, 1d sequences, at most 128 channels, Nq >= 1, capacity >= 1 and "
                     "1 <= g <= 128 with g = Hq / Hk")


def _ragged_forward(what, prefill, Q, K, V, k_lens, tail_causal, returning_l_m, k_scale, v_scale, window_size,
                    draft_mask=None):
    """``ragged_1d`` (``prefill`` False) and ``ragged_prefill_1d``: one validation, the entry points differ."""
    Qb, Qs, Q_ch, Kb, Ks, V_ch, g = verify_grouped_shapes(1, Q.shape, K.shape, V.shape)
    dt = _dtype_id(Q, True)
    kv_per_len = int(Kb[-1]) if Kb else 1
    fp8 = _kv_cache_scales("K and V", Q, K, V, kv_per_len, k_scale, v_scale)
    if not isinstance(k_lens, torch.Tensor) or k_lens.dtype != torch.int32:
        raise TypeError(f"k_lens must be an int32 tensor, got {getattr(k_lens, 'dtype', type(k_lens).__name__)}")
    batch = Qb[:-1]
    if tuple(k_lens.shape) != tuple(batch):
        raise InvalidArgumentError("The shape of k_lens should be the batch shape without the heads, but k_lens_shape = "
                                   + _shape_str(k_lens.shape) + ", batch_shape = " + _shape_str(batch)
                                   + " were received")
    if k_lens.device != Q.device:
        raise InvalidArgumentError("k_lens must be on the device of Q, K and V")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (Q, K, V)):
        raise RuntimeError(what + " is inference only and has no gradient; call it under torch.no_grad() or "
                           "detach its inputs")
    window = _decode_window(what, window_size, tail_causal, int(Qs[0]))
    mask = _decode_mask(what, draft_mask, tail_causal, window_size, Q, batch, int(Qs[0]))
    prob = _lib.make_problem(dt, _lib.FULL, 1, _lib.NONE_FRONT, _prod(Qb), Qs, Ks, Q_ch, V_ch)
    L = _lib.lib()
    plan_name, ws_name, forward_name = decode_entry_points("ragged", _decode_form(prefill, window, mask), fp8)
    own = (prob, g) + (() if window is None else (window,))  # the plan functions' own arguments
    plan = (ctypes.c_int32 * 8)()
    st = getattr(L, plan_name)(*own, plan)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    if plan[0] == 0:
        raise NotImplementedError(what + ": outside the fused envelope ("
                                  + (_PREFILL_ENVELOPE if prefill else _RAGGED_ENVELOPE) + "), got Q_shape = "
                                  + _shape_str(Q.shape) + ", K_shape = " + _shape_str(K.shape) + ", V_shape = "
                                  + _shape_str(V.shape))
    _check_device_tensors(Q, K, V)
    Q, K, V, k_lens = Q.contiguous(), K.contiguous(), V.contiguous(), k_lens.contiguous()
    O = torch.empty(Qb + (V_ch,) + Qs, dtype=Q.dtype, device=Q.device)
    l = torch.empty(Qb + Qs, dtype=torch.float32, device=Q.device)
    m = torch.empty(Qb + Qs, dtype=Q.dtype, device=Q.device)
    ws_bytes = int(getattr(L, ws_name)(*own))
    with torch.cuda.device(Q.device):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=Q.device)
        st = getattr(L, forward_name)(_stream_handle(Q.device), prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                      *_scale_ptrs(fp8, k_scale, v_scale), k_lens.data_ptr(), kv_per_len,
                                      mask.data_ptr() if mask is not None else int(bool(tail_causal)) if window is None
                                      else window, O.data_ptr(),
                                      l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    return (O, l, m) if returning_l_m else O


# ----------------------------------------------------------------------------
# Paged few-query forward: decode over a pool of K/V pages with a block table on the device
# (include/fa_api.h, "Paged few-query forward")
# ----------------------------------------------------------------------------
_PAGE_CONDITION = "the page size (the last axis of K_pool and V_pool) must be a multiple of 64 keys"


def paged_1d(Q, K_pool, V_pool, block_table, k_lens, tail_causal=False, returning_l_m=False, k_scale=None,
             v_scale=None, window_size=None, draft_mask=None):
    """``ragged_1d`` over a paged K/V cache: Q ``batch + (Hq, C, Nq)``, ``K_pool`` ``[num_pages, Hk, C, page]``,
    ``V_pool`` ``[num_pages, Hk, Cv, page]`` with Hq = g * Hk read from the shapes, ``block_table`` an int32 tensor
    ``batch + (max_pages,)`` and ``k_lens`` an int32 tensor of shape ``batch``, both on the device of Q.  A page
    holds ``page`` consecutive key positions of all Hk heads of one sequence; ``block_table[s, p]`` is the pool page
    with keys ``[p * page, (p + 1) * page)`` of sequence s, which attends its first ``k_lens[s]`` keys, clamped to
    ``[0, max_pages * page]``.  ``tail_causal`` and the rows without a key are ``ragged_1d``'s.  Sequences may share
    pages (a common prefix).

    Neither tensor is read on the host: no synchronisation, and a captured graph may be replayed after ``k_lens`` or
    ``block_table`` was overwritten in place.  Table entries of pages without a live key are never loaded; a loaded
    entry is clamped to ``[0, num_pages - 1]``.  Appending token ``new`` (``[Hk, C]``) of sequence s at position
    ``pos`` (a device tensor) needs no host read either, it is an ``index_put`` with device indices::

        K_pool[block_table[s, pos // page], :, :, pos % page] = new

    An FP8 cache: pools of dtype ``torch.float8_e4m3fn`` (or the same bytes as ``torch.uint8``) with Q float16, and
    ``k_scale`` / ``v_scale`` float32 tensors of shape ``(Hk,)`` on the device of Q, or None for 1.0, as in
    ``ragged_1d``; they too may be overwritten in place between replays.  The append quantizes the token with the
    pool's scales, still without a host read::

        new8, _ = quantize_kv_fp8(new, head_axis=0, scale=k_scale)
        K_pool[block_table[s, pos // page], :, :, pos % page] = new8

    ``paged_append_1d`` is both recipes as one kernel, for K and V of a whole batch and any number of new tokens.

    A sliding window: ``window_size`` = W >= 1 (None: no window), with ``ragged_1d``'s rule: Nq > 1 requires
    ``tail_causal=True``, and query i at position ``pos = k_lens[s] - Nq + i`` sees the W keys
    ``max(0, pos - W + 1) <= j <= pos``.  Work, workspace and time follow W + Nq - 1, not the capacity; ``W >= cap``
    is the tail-causal call itself.  With ``lo = max(0, k_lens[s] - Nq - W + 1)``: keys below ``lo // 64 * 64`` are
    never read, and the table entries of pages wholly below that key are never loaded, like those past the last
    live page, so such pages may be freed and reused and their entries may hold anything.  The at most 63 keys
    between ``lo // 64 * 64`` and ``lo`` are read and masked: they must be finite (they lie on a page the
    sequence still owns).  Attention sinks (the first S keys stay visible) compose from two calls and
    ``merge_partials``::

        O1, l1, m1 = paged_1d(Q, K_pool, V_pool, table, k_lens, tail_causal=True, returning_l_m=True, window_size=W)
        O2, l2, m2 = paged_1d(Q, K_pool, V_pool, table, k_lens.clamp(max=S), returning_l_m=True)
        O, l, m = merge_partials([O1, O2], [l1, l2], [m1, m2])

    (exact where the two key sets are disjoint: S <= k_lens - Nq - W + 1).

    A tree of draft tokens: ``draft_mask``, an int32 tensor ``batch + (Nq, ceil(Nq / 32))`` of raw bits on the device
    of Q, with ``ragged_1d``'s rule (``tail_causal=True`` required, no ``window_size``): query i sees the keys below
    ``k_lens[s] - Nq`` and the draft slots its row names.  One call replaces a context call, a gather of the draft
    keys out of the pages, a masked attention over them and ``merge_partials``; the mask may be overwritten in place
    between replays like ``k_lens`` and ``block_table``.  ``draft_mask_from_parents`` builds it from a forest.

    Inference only (no gradient); float16 only; the page size must be a multiple of 64; outside the envelope the
    call raises NotImplementedError (there is no gather fallback).  More queries than the envelope's
    g * next_pow2(Nq) <= 128: ``paged_prefill_1d``.  Returns ``O`` or ``(O, l, m)``."""
    return _paged_forward("paged_1d", False, Q, K_pool, V_pool, block_table, k_lens, tail_causal, returning_l_m, k_scale,
                          v_scale, window_size, draft_mask)


def paged_prefill_1d(Q, K_pool, V_pool, block_table, k_lens, tail_causal=False, returning_l_m=False, k_scale=None,
                     v_scale=None):
    """``paged_1d`` for any number of queries (chunked prefill against the paged cache, long speculative drafts):
    the same pools, block table, lengths, ``tail_causal`` rule, empty rows, FP8 pools and scales, with Nq >= 1
    unbounded and 1 <= g <= 128.  The queries are worked in blocks of P = the largest power of two with
    g * P <= 128; where one block holds them all the call is ``paged_1d`` itself, bit for bit.  There is no
    ``window_size``.  (Under a sliding window: ``paged_window_prefill_1d``.)  The new tokens' keys are appended to
    the pools first (``paged_1d`` shows how), so that ``k_lens`` counts them; ``paged_append_1d`` does it in one
    call, with this function's ``k_lens`` and the real tokens right-aligned as the queries are.

    A batch that mixes prefill with decode right-aligns each sequence's real queries in the Nq slots (with
    ``tail_causal`` the last slot is the sequence's last position).  The padding queries in front compute earlier
    positions' rows, or empty rows where they lie before position 0; the caller ignores them.

    Nothing is read on the host; table entries of pages without a live key are never loaded and loaded entries are
    clamped.  Inference only; float16 only; the page size must be a multiple of 64; outside the envelope the call
    raises NotImplementedError.  Returns ``O`` or ``(O, l, m)``."""
    return _paged_forward("paged_prefill_1d", True, Q, K_pool, V_pool, block_table, k_lens, tail_causal, returning_l_m,
                          k_scale, v_scale, None)


def paged_window_prefill_1d(Q, K_pool, V_pool, block_table, k_lens, window_size, returning_l_m=False, k_scale=None,
                            v_scale=None):
    """``paged_1d`` under a sliding window for any number of queries (chunked prefill of local-attention layers
    against the paged cache): the same pools, block table, lengths, empty rows, FP8 pools and scales, with Nq >= 1
    unbounded and 1 <= g <= 128.  ``window_size`` = W is a required int >= 1 (clamped to 2^31 - 1), and the rule,
    the blocks and the two bit-for-bit delegations (``W >= cap``: ``paged_prefill_1d(..., tail_causal=True)``; one
    block: ``paged_1d(..., tail_causal=True, window_size=W)``) are ``ragged_window_prefill_1d``'s.  The new tokens'
    keys are appended first (``paged_append_1d``), so that ``k_lens`` counts them.

    Lengths, table and scales are read on the device, never on the host: no synchronisation, and the call may be
    replayed from a captured graph after any of them was overwritten in place.  Queries of a mixed batch are
    right-aligned in the Nq slots.  With ``lo = max(0, k_lens[s] - Nq - W + 1)``, the call's lowest window start:
    keys below ``lo // 64 * 64`` are never read, and the table entries of pages wholly below that key are never
    loaded, like those past the last live page, so such pages may be freed and reused and their entries may hold
    anything; loaded entries are clamped.  The up to 63 keys between ``lo // 64 * 64`` and ``lo`` are read and
    masked, so they must be finite.  Attention sinks compose from a second call and ``merge_partials``, as in
    ``paged_1d``.

    Inference only; float16 only; the page size must be a multiple of 64; outside the envelope the call raises
    NotImplementedError.  Returns ``O`` or ``(O, l, m)``."""
    return _paged_forward("paged_window_prefill_1d", True, Q, K_pool, V_pool, block_table, k_lens, True, returning_l_m,
                          k_scale, v_scale, _required_window(window_size))


def _paged_forward(what, prefill, Q, K_pool, V_pool, block_table, k_lens, tail_causal, returning_l_m, k_scale, v_scale,
                   window_size, draft_mask=None):
    """``paged_1d`` (``prefill`` False) and ``paged_prefill_1d``: one validation, the entry points differ."""
    if len(K_pool.shape) != 4 or len(V_pool.shape) != 4:
        raise InvalidArgumentError("K_pool and V_pool should be [num_pages, Hk, channels, page], but K_pool_shape = "
                                   + _shape_str(K_pool.shape) + ", V_pool_shape = " + _shape_str(V_pool.shape)
                                   + " were received")
    num_pages, hk, k_ch, page = (int(x) for x in K_pool.shape)
    if (int(V_pool.shape[0]), int(V_pool.shape[1]), int(V_pool.shape[3])) != (num_pages, hk, page):
        raise InvalidArgumentError("K_pool and V_pool should agree in num_pages, Hk and page, but K_pool_shape = "
                                   + _shape_str(K_pool.shape) + ", V_pool_shape = " + _shape_str(V_pool.shape)
                                   + " were received")
    v_ch = int(V_pool.shape[2])
    if len(Q.shape) < 3:
        raise InvalidArgumentError("Q should be batch + (Hq, C, Nq), but Q_shape = " + _shape_str(Q.shape)
                                   + " was received")
    batch, hq, q_ch, nq = tuple(Q.shape[:-3]), int(Q.shape[-3]), int(Q.shape[-2]), int(Q.shape[-1])
    if q_ch != k_ch:
        raise InvalidArgumentError("The channels of Q and K_pool should be the same, but Q_shape = "
                                   + _shape_str(Q.shape) + ", K_pool_shape = " + _shape_str(K_pool.shape)
                                   + " were received")
    if num_pages < 1 or hk < 1 or hq % hk != 0:
        raise InvalidArgumentError("The heads of Q should be a multiple of the heads of a page, and the pools should "
                                   "hold a page, but Q_shape = " + _shape_str(Q.shape) + ", K_pool_shape = "
                                   + _shape_str(K_pool.shape) + " were received")
    dt = _dtype_id(Q, True)
    fp8 = _kv_cache_scales("K_pool and V_pool", Q, K_pool, V_pool, hk, k_scale, v_scale)
    for name, t in (("block_table", block_table), ("k_lens", k_lens)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"{name} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(block_table.shape[:-1]) != batch or len(block_table.shape) != len(batch) + 1 or block_table.shape[-1] < 1:
        raise InvalidArgumentError("The shape of block_table should be the batch shape without the heads plus "
                                   "(max_pages,), but block_table_shape = " + _shape_str(block_table.shape)
                                   + ", batch_shape = " + _shape_str(batch) + " were received")
    if tuple(k_lens.shape) != batch:
        raise InvalidArgumentError("The shape of k_lens should be the batch shape without the heads, but k_lens_shape = "
                                   + _shape_str(k_lens.shape) + ", batch_shape = " + _shape_str(batch)
                                   + " were received")
    if block_table.device != Q.device or k_lens.device != Q.device:
        raise InvalidArgumentError("block_table and k_lens must be on the device of Q, K_pool and V_pool")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (Q, K_pool, V_pool)):
        raise RuntimeError(what + " is inference only and has no gradient; call it under torch.no_grad() or "
                           "detach its inputs")
    if page < 1 or page % 64 != 0:
        raise NotImplementedError(what + ": " + _PAGE_CONDITION + ", got page = " + str(page))
    g, max_pages = hq // hk, int(block_table.shape[-1])
    cap = max_pages * page
    if cap > 2 ** 30:
        raise InvalidArgumentError("The capacity max_pages * page = " + str(cap) + " is above 2^30 keys")
    window = _decode_window(what, window_size, tail_causal, nq)
    mask = _decode_mask(what, draft_mask, tail_causal, window_size, Q, batch, nq)
    prob = _lib.make_problem(dt, _lib.FULL, 1, _lib.NONE_FRONT, _prod(batch) * hq, (nq,), (cap,), q_ch, v_ch)
    L = _lib.lib()
    plan_name, ws_name, forward_name = decode_entry_points("paged", _decode_form(prefill, window, mask), fp8)
    own = (prob, g, page) + (() if window is None else (window,))  # the plan functions' own arguments
    plan = (ctypes.c_int32 * 8)()
    st = getattr(L, plan_name)(*own, plan)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    if plan[0] == 0:
        raise NotImplementedError(what + ": outside the fused envelope ("
                                  + (_PREFILL_ENVELOPE if prefill else _RAGGED_ENVELOPE) + "; and "
                                  + _PAGE_CONDITION + "), got Q_shape = " + _shape_str(Q.shape) + ", K_pool_shape = "
                                  + _shape_str(K_pool.shape) + ", V_pool_shape = " + _shape_str(V_pool.shape))
    _check_device_tensors(Q, K_pool, V_pool)
    Q, K_pool, V_pool = Q.contiguous(), K_pool.contiguous(), V_pool.contiguous()
    block_table, k_lens = block_table.contiguous(), k_lens.contiguous()
    O = torch.empty(batch + (hq, v_ch, nq), dtype=Q.dtype, device=Q.device)
    l = torch.empty(batch + (hq, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty(batch + (hq, nq), dtype=Q.dtype, device=Q.device)
    ws_bytes = int(getattr(L, ws_name)(*own))
    with torch.cuda.device(Q.device):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=Q.device)
        st = getattr(L, forward_name)(_stream_handle(Q.device), prob, g, Q.data_ptr(), K_pool.data_ptr(),
                                      V_pool.data_ptr(), *_scale_ptrs(fp8, k_scale, v_scale), block_table.data_ptr(),
                                      max_pages, page, num_pages, k_lens.data_ptr(), hk,
                                      mask.data_ptr() if mask is not None else int(bool(tail_causal)) if window is None
                                      else window, O.data_ptr(),
                                      l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
    if st != _lib.FA_OK:
        _raise_status(st, "Forward")
    return (O, l, m) if returning_l_m else O


# ----------------------------------------------------------------------------
# Fused K/V append: the write side of the ragged and the paged cache, fp16 or FP8
# (include/fa_api.h, "Fused K/V append")
# ----------------------------------------------------------------------------
def ragged_append_1d(K, V, K_new, V_new, k_lens, new_lens=None, k_scale=None, v_scale=None):
    """Appends new tokens' keys and values to the padded cache of ``ragged_1d``, in place, with one kernel: K
    ``batch + (Hk, C, cap)``, V ``batch + (Hk, Cv, cap)``, float16 or an FP8 cache (``float8_e4m3fn`` or ``uint8``);
    ``K_new`` ``batch + (Hk, C, Nnew)`` and ``V_new`` ``batch + (Hk, Cv, Nnew)`` float16 (made contiguous if they are
    not); ``k_lens`` and ``new_lens`` int32 tensors of shape ``batch`` on the cache's device.

    ``k_lens[s]`` is the length AFTER the append, clamped to [0, cap]: the tensor this step's attention call takes.
    ``new_lens[s]`` (None: Nnew for every sequence) is the number of real new tokens of sequence s, clamped to
    [0, min(Nnew, k_lens[s])] and RIGHT-ALIGNED in the Nnew slots, as the queries of ``ragged_prefill_1d`` are: the
    last n slots go to positions ``k_lens[s] - n .. k_lens[s] - 1``.  The slots in front are padding and are never
    read.  Only those positions are written; nothing else in the cache changes.

    An FP8 cache stores ``e4m3fn(float32(x) / scale[h])``, rounded to nearest even and saturated at +-448: for every
    finite or infinite x the bytes of ``quantize_kv_fp8(x, scale=...)``.  ``k_scale`` / ``v_scale`` are float32 tensors
    of shape ``(Hk,)`` on the device, or None for 1.0; a float16 cache takes no scale.

    Nothing is read on the host: no synchronisation, and a captured graph may be replayed after any of the tensors
    was overwritten in place.  The call runs on the current stream, so a forward called after it sees the tokens.  It
    does not change ``k_lens`` or ``new_lens`` and computes no scales.  The cache must be contiguous (a copy would
    silently take the write).  Inference only.  Returns None."""
    if len(K.shape) < 3 or len(V.shape) != len(K.shape):
        raise InvalidArgumentError("K and V should be batch + (Hk, channels, cap), but K_shape = " + _shape_str(K.shape)
                                   + ", V_shape = " + _shape_str(V.shape) + " were received")
    batch, hk, k_ch, cap = tuple(K.shape[:-3]), int(K.shape[-3]), int(K.shape[-2]), int(K.shape[-1])
    if tuple(V.shape[:-2]) != batch + (hk,) or int(V.shape[-1]) != cap:
        raise InvalidArgumentError("K and V should agree in the batch shape, Hk and cap, but K_shape = "
                                   + _shape_str(K.shape) + ", V_shape = " + _shape_str(V.shape) + " were received")
    v_ch = int(V.shape[-2])
    n_new = _append_checks("ragged_append_1d", "K and V", K, V, K_new, V_new, batch, hk, k_ch, v_ch, (("k_lens", k_lens),),
                           new_lens, k_scale, v_scale)
    if cap > 2 ** 30:
        raise InvalidArgumentError("The capacity " + str(cap) + " is above 2^30 keys")
    _append_call("ragged", K, V, K_new, V_new, batch, hk, k_ch, v_ch, n_new, cap, (), k_lens, new_lens, k_scale, v_scale)


def paged_append_1d(K_pool, V_pool, K_new, V_new, block_table, k_lens, new_lens=None, k_scale=None, v_scale=None):
    """``ragged_append_1d`` into the page pools of ``paged_1d``: ``K_pool`` ``[num_pages, Hk, C, page]``, ``V_pool``
    ``[num_pages, Hk, Cv, page]``, float16 or FP8; ``K_new`` ``batch + (Hk, C, Nnew)``, ``V_new``
    ``batch + (Hk, Cv, Nnew)`` float16; ``block_table`` int32 ``batch + (max_pages,)``; ``k_lens`` (the lengths AFTER
    the append, clamped to ``[0, max_pages * page]``) and ``new_lens`` int32 of shape ``batch``.  Position ``pos`` of
    sequence s goes to ``K_pool[block_table[s, pos // page], :, :, pos % page]``: the docstring recipe of ``paged_1d``
    for a whole batch, any number of tokens and pages, and the FP8 quantization, in one kernel.

    Only the table entries of pages that receive a new position are loaded, each clamped to ``[0, num_pages - 1]``:
    every store lies inside the pools.  A page that no written position names (a shared prefix) is untouched; two
    sequences that name one page at a written position race, which is the caller's bug.  The call allocates no
    pages, changes neither the table nor the lengths, computes no scales and does no copy-on-write.

    Lengths, ``new_lens``, scales, FP8 rounding, graph replay, the stream and the contiguous pools: as in
    ``ragged_append_1d``.  The page size must be a multiple of 64 (NotImplementedError otherwise: nothing here can
    read such a pool).  Inference only.  Returns None."""
    if len(K_pool.shape) != 4 or len(V_pool.shape) != 4:
        raise InvalidArgumentError("K_pool and V_pool should be [num_pages, Hk, channels, page], but K_pool_shape = "
                                   + _shape_str(K_pool.shape) + ", V_pool_shape = " + _shape_str(V_pool.shape)
                                   + " were received")
    num_pages, hk, k_ch, page = (int(x) for x in K_pool.shape)
    if (int(V_pool.shape[0]), int(V_pool.shape[1]), int(V_pool.shape[3])) != (num_pages, hk, page):
        raise InvalidArgumentError("K_pool and V_pool should agree in num_pages, Hk and page, but K_pool_shape = "
                                   + _shape_str(K_pool.shape) + ", V_pool_shape = " + _shape_str(V_pool.shape)
                                   + " were received")
    v_ch = int(V_pool.shape[2])
    if num_pages < 1:
        raise InvalidArgumentError("The pools should hold a page, but K_pool_shape = " + _shape_str(K_pool.shape)
                                   + " was received")
    batch = tuple(K_new.shape[:-3]) if len(getattr(K_new, "shape", ())) >= 3 else ()
    n_new = _append_checks("paged_append_1d", "K_pool and V_pool", K_pool, V_pool, K_new, V_new, batch, hk, k_ch, v_ch,
                           (("block_table", block_table), ("k_lens", k_lens)), new_lens, k_scale, v_scale)
    if page < 1 or page % 64 != 0:
        raise NotImplementedError("paged_append_1d: " + _PAGE_CONDITION + ", got page = " + str(page))
    max_pages = int(block_table.shape[-1])
    cap = max_pages * page
    if cap > 2 ** 30:
        raise InvalidArgumentError("The capacity max_pages * page = " + str(cap) + " is above 2^30 keys")
    _append_call("paged", K_pool, V_pool, K_new, V_new, batch, hk, k_ch, v_ch, n_new, cap,
                 (block_table, max_pages, page, num_pages), k_lens, new_lens, k_scale, v_scale)


def _append_checks(what, caches, K, V, K_new, V_new, batch, hk, k_ch, v_ch, int_tensors, new_lens, k_scale, v_scale):
    """The checks that ``ragged_append_1d`` and ``paged_append_1d`` share, after those of the cache's own shape and
    before the page size's: the new tokens, the dtypes and scales, the int32 tensors, grad mode, the contiguous
    cache.  Returns Nnew."""
    for name, t in (("K_new", K_new), ("V_new", V_new)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float16:
            raise TypeError(f"{name} must be a float16 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    n_new = int(K_new.shape[-1]) if len(K_new.shape) >= 1 else 0
    if tuple(K_new.shape) != batch + (hk, k_ch, n_new) or tuple(V_new.shape) != batch + (hk, v_ch, n_new):
        raise InvalidArgumentError("K_new and V_new should be batch + (Hk, C, Nnew) and batch + (Hk, Cv, Nnew) with "
                                   "batch_shape = " + _shape_str(batch) + ", Hk = " + str(hk) + ", C = " + str(k_ch)
                                   + ", Cv = " + str(v_ch) + ", but K_new_shape = " + _shape_str(K_new.shape)
                                   + ", V_new_shape = " + _shape_str(V_new.shape) + " were received")
    _kv_cache_scales(caches, K_new, K, V, hk, k_scale, v_scale, q="K_new and V_new")
    int_tensors = int_tensors + ((("new_lens", new_lens),) if new_lens is not None else ())
    for name, t in int_tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"{name} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    for name, t in int_tensors:
        if name == "block_table":
            if tuple(t.shape[:-1]) != batch or len(t.shape) != len(batch) + 1 or t.shape[-1] < 1:
                raise InvalidArgumentError("The shape of block_table should be the batch shape without the heads plus "
                                           "(max_pages,), but block_table_shape = " + _shape_str(t.shape)
                                           + ", batch_shape = " + _shape_str(batch) + " were received")
        elif tuple(t.shape) != batch:
            raise InvalidArgumentError(f"The shape of {name} should be the batch shape without the heads, but {name}_shape = "
                                       + _shape_str(t.shape) + ", batch_shape = " + _shape_str(batch) + " were received")
    if any(t.device != K.device for t in (V, K_new, V_new)) or any(t.device != K.device for _, t in int_tensors):
        raise InvalidArgumentError(", ".join(n for n, _ in int_tensors) + f", K_new and V_new must be on the device of {caches}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (K, V, K_new, V_new)):
        raise RuntimeError(what + " is inference only and has no gradient; call it under torch.no_grad() or "
                           "detach its inputs")
    if not K.is_contiguous() or not V.is_contiguous():
        raise InvalidArgumentError(f"{what}: {caches} must be contiguous: the append writes in place, and a contiguous "
                                   "copy would silently take the write")
    return n_new


def _append_call(cache, K, V, K_new, V_new, batch, hk, k_ch, v_ch, n_new, cap, paged_args, k_lens, new_lens, k_scale,
                 v_scale):
    """The device check (last, as in the forwards) and the C call of an append."""
    _check_device_tensors(K, V, K_new, V_new)
    fp8 = K.dtype in _FP8_CACHE_DTYPES
    K_new, V_new, k_lens = K_new.contiguous(), V_new.contiguous(), k_lens.contiguous()
    new_lens = new_lens.contiguous() if new_lens is not None else None
    if paged_args:
        paged_args = (paged_args[0].contiguous().data_ptr(),) + tuple(paged_args[1:])
    with torch.cuda.device(K.device):
        st = getattr(_lib.lib(), _lib.append_entry_point(cache, fp8))(
            _stream_handle(K.device), _prod(batch), hk, k_ch, v_ch, n_new, cap, K_new.data_ptr(), V_new.data_ptr(),
            K.data_ptr(), V.data_ptr(), *_scale_ptrs(fp8, k_scale, v_scale), *paged_args, k_lens.data_ptr(),
            new_lens.data_ptr() if new_lens is not None else None)
    if st != _lib.FA_OK:
        _raise_status(st, "append")


# ----------------------------------------------------------------------------
# Op-name mirror of the TF-generated wrappers (REGISTER_OP names, snake_cased)
# ----------------------------------------------------------------------------
def _make_forward_op(policy, seq_dims, float16):
    def op(q, k, v, sync_mode, window_size=1, log2_stride_size=0, is_causal=False):
        return attention_forward(policy, seq_dims, q, k, v, sync_mode, window_size, log2_stride_size, is_causal,
                                 float16_op=float16)
    return op


def _make_backward_op(policy, seq_dims, float16):
    def op(q, k, v, o, l, m, d_o, sync_mode, window_size=1, log2_stride_size=0, is_causal=False):
        return attention_backward(policy, seq_dims, q, k, v, o, l, m, d_o, sync_mode, window_size,
                                  log2_stride_size, is_causal, float16_op=float16)
    return op


def estimate_forward_flops(policy, seq_dims, q_shape, k_shape, v_shape, sync_mode="none_front", window_size=1,
                           log2_stride_size=0, is_causal=False) -> float:
    """Estimate{Full,Causal,Local}AttentionForward{1,2}dFlops (flash_attention_forward.cc:217-245):
    algorithmic 2*(d+v_d)*allowed_pairs (not tile-issued work)."""
    sid = _sync_mode_id(sync_mode)
    Qb, Qs, Q_ch, _, Ks, _, _, _, V_ch = verify_and_extract_shapes(seq_dims, q_shape, k_shape, v_shape)
    prob = _lib.make_problem(_lib.F32, _POLICIES[policy], seq_dims, sid, _prod(Qb), Qs, Ks, Q_ch, V_ch,
                             window_size, log2_stride_size, is_causal)
    return float(_lib.lib().fa_estimate_forward_flops(prob))


def _make_flops_op(policy, seq_dims):
    def op(q_shape, k_shape, v_shape, dtype=None, sync_mode="none_front", window_size=1, log2_stride_size=0,
           is_causal=False):
        return estimate_forward_flops(policy, seq_dims, q_shape, k_shape, v_shape, sync_mode, window_size,
                                      log2_stride_size, is_causal)
    return op


_ops = {}
for _pol in ("full", "causal", "local"):
    for _sd in (1, 2):
        for _f16 in (True, False):
            suffix = "_float16" if _f16 else ""
            _ops[f"{_pol}_attention_forward{_sd}d{suffix}"] = _make_forward_op(_pol, _sd, _f16)
            _ops[f"{_pol}_attention_backward{_sd}d{suffix}"] = _make_backward_op(_pol, _sd, _f16)
        _ops[f"estimate_{_pol}_attention_forward{_sd}d_flops"] = _make_flops_op(_pol, _sd)
_fa_kernel = SimpleNamespace(**_ops)

# gradient dispatch table, as registered with @ops.RegisterGradient (flash_attention.py:392-471)
_OP_RE = re.compile(r".+(?P<ndim>\dd)(?P<f16>Float16)?$")


def gradient_op_for(op_type: str):
    """Maps a forward op type name (e.g. 'CausalAttentionForward1dFloat16') to its backward op."""
    m = re.match(r"(Full|Causal|Local)AttentionForward", op_type)
    match = _OP_RE.match(op_type)
    if not m or not match:
        raise ValueError(f'Unsupported op "{op_type}"')
    g = match.groupdict()
    name = f"{m.group(1).lower()}_attention_backward{g['ndim']}{'_float16' if g['f16'] else ''}"
    return getattr(_fa_kernel, name)


# ----------------------------------------------------------------------------
# The 'flops' statistic of each forward op (flash_attention.py:475-562 registers these with
# ops.RegisterStatistics, so TF's profiler reports the op's algorithmic FLOPs)
# ----------------------------------------------------------------------------
_STAT_OPS = tuple(f"{p}AttentionForward{n}d{f}" for p in ("Full", "Causal", "Local") for n in (1, 2)
                  for f in ("", "Float16"))


def forward_flops_statistics(op_type: str, q_shape, k_shape, v_shape, attrs) -> float:
    """The statistic the reference computes for a forward node (_estimate_{full,causal,local}_attention_
    forward_flops, flash_attention.py:498-562): the op's Estimate*Flops over the node's Q/K/V shapes with
    its sync_mode attr, and window_size / log2_stride_size / is_causal for the local ops.  Raises
    ValueError('Unsupported op "..."') for any other op name, as the reference does."""
    m = re.match(r"(Full|Causal|Local)AttentionForward(\d)d(Float16)?$", op_type)
    if not m or m.group(2) not in ("1", "2"):
        raise ValueError(f'Unsupported op "{op_type}"')
    policy, seq_dims = m.group(1).lower(), int(m.group(2))
    kw = {"sync_mode": attrs["sync_mode"]}
    if policy == "local":
        kw.update(window_size=int(attrs["window_size"]), log2_stride_size=int(attrs["log2_stride_size"]),
                  is_causal=bool(attrs["is_causal"]))
    return estimate_forward_flops(policy, seq_dims, tuple(q_shape), tuple(k_shape), tuple(v_shape), **kw)


def register_tf_statistics() -> bool:
    """With TensorFlow importable (the TF-ROCm op library of tf_op/ loaded), register
    forward_flops_statistics as the 'flops' statistic of the 12 forward ops, as importing the
    reference module does.  Returns False (nothing registered) when TensorFlow is absent."""
    try:
        from tensorflow.python.framework import ops as tf_ops  # noqa: WPS433 (optional dependency)
    except ImportError:
        return False

    def _stat(graph, node):
        def tensor(name):
            return graph.get_tensor_by_name(name if ":" in name else name + ":0")
        q, k, v = (tensor(node.input[i]) for i in range(3))
        attrs = {"sync_mode": node.attr["sync_mode"].s.decode()}
        if node.op.startswith("Local"):
            attrs.update(window_size=node.attr["window_size"].i, log2_stride_size=node.attr["log2_stride_size"].i,
                         is_causal=node.attr["is_causal"].b)
        flops = forward_flops_statistics(node.op, q.shape.as_list(), k.shape.as_list(), v.shape.as_list(), attrs)
        return tf_ops.OpStats("flops", flops)

    for name in _STAT_OPS:
        tf_ops.RegisterStatistics(name, "flops")(_stat)
    return True

