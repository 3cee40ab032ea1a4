"""GPU tests of the merge of attention partials and of combined attention.

The merge kernel alone runs on synthetic partials (no attention call) against a numpy float64 evaluation of
the formulas of include/fa_api.h; fa_accumulate_parts against a float64 sum.  Combined attention (forward
and backward) is checked against a dense float64 computation on the CPU: the parts' keys concatenated,
their masks (oracle.problem_mask of each part's own problem) concatenated, one softmax at scale 1/sqrt(d),
gradients taken analytically.  No reference comes from the code under test.

Tolerances (tests/gate.py):
  merge alone   O: gate.plain_bound at the dtype's forward TOL (the inputs are exact here); l: the dtype's
                forward rtol, relative; m: exactly the maximum.
  combined      O: the forward gate's plain bound + u_T * max|V| (the partial O_i are stored in T and
                |O_i| <= max|V|); l and m: run_case's checks; gradients: the plain backward bound, plus
                N * u_T * max_i max|dQ_i| for dQ (the dQ_i are stored in T before the fp32 sum).
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import fa_oracle as O
from tests import gate
from tests.gate import TOL, U_ROUND
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

DTYPES = [np.float16, np.float32, np.float64]
DT_ID = {np.float16: _lib.F16, np.float32: _lib.F32, np.float64: _lib.F64}
_id = lambda t: np.dtype(t).name  # noqa: E731


def _dev():
    return torch.device("cuda:0")


def _to_dev(x, misalign=False):
    """x on the device; with ``misalign`` at a data pointer one element past an aligned allocation."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(_dev())
    if misalign:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=_dev())
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _empty_like(x, misalign=False):
    return _to_dev(np.zeros_like(x), misalign)


# ------------------------------------------------------------------------------------------------
# the merge kernel alone
# ------------------------------------------------------------------------------------------------
def synthetic_partials(dtype, n, b, v_d, nq, seed, empty=True):
    """n partials in the forwards' format: O_i in U(-2, 2), m_i over +-20, l_i in [1, 50].  With ``empty``
    about a fifth of the (part, row) pairs are empty (O = 0, l = 0, m = NegInfApprox), and rows 5, 11, 17, ...
    of every slice are empty in every part."""
    rng = np.random.default_rng(seed)
    LT = O.l_dtype_for(dtype)
    Os = [rng.uniform(-2, 2, (b, v_d, nq)).astype(dtype) for _ in range(n)]
    ms = [rng.uniform(-20, 20, (b, nq)).astype(dtype) for _ in range(n)]
    ls = [rng.uniform(1, 50, (b, nq)).astype(LT) for _ in range(n)]
    if empty:
        for i in range(n):
            gone = rng.random((b, nq)) < 0.2
            gone[:, 5::6] = True
            make_empty(Os[i], ls[i], ms[i], gone)
    return Os, ls, ms


def make_empty(Oi, li, mi, rows):
    """rows [b, nq] bool: what a forward writes for a row that attends nothing."""
    Oi[np.broadcast_to(rows[:, None, :], Oi.shape)] = 0
    li[rows] = 0
    mi[rows] = O.neg_inf_approx(mi.dtype)


def merge_reference(Os, ls, ms):
    """The formulas of include/fa_api.h in float64.  Returns (O, L, m (float64 of the exact T value), live)."""
    l64 = np.stack([x.astype(np.float64) for x in ls])
    m64 = np.stack([x.astype(np.float64) for x in ms])
    o64 = np.stack([x.astype(np.float64) for x in Os])
    live = l64 != 0
    m = np.where(live, m64, -np.inf).max(axis=0)
    any_live = live.any(axis=0)
    m_safe = np.where(any_live, m, 0.0)
    e = np.where(live, l64 * np.exp(np.where(live, m64 - m_safe, 0.0)), 0.0)
    L = e.sum(axis=0)
    w = e / np.where(any_live, L, 1.0)
    return (w[:, :, None, :] * o64).sum(axis=0), L, m_safe, any_live


def call_merge(dtype, Os, ls, ms, misalign=False):
    """fa_merge_partials through ctypes on device copies; returns numpy (O, l, m)."""
    dOs, dls, dms = ([_to_dev(x, misalign) for x in xs] for xs in (Os, ls, ms))
    out = [_empty_like(x, misalign) for x in (Os[0], ls[0], ms[0])]
    b, v_d, nq = Os[0].shape
    st = _lib.lib().fa_merge_partials(
        torch.cuda.current_stream(_dev()).cuda_stream, DT_ID[dtype], b, nq, v_d, len(Os),
        _lib.pointer_array([t.data_ptr() for t in dOs]), _lib.pointer_array([t.data_ptr() for t in dls]),
        _lib.pointer_array([t.data_ptr() for t in dms]), *(t.data_ptr() for t in out))
    assert st == _lib.FA_OK, _lib.last_error()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_merge(dtype, Os, ls, ms, got, tag):
    og, lg, mg = got
    o_ref, L, m, any_live = merge_reference(Os, ls, ms)
    rtol, atol = TOL[dtype]["fwd"]
    assert np.isfinite(og.astype(np.float64)).all(), tag
    err = np.abs(og.astype(np.float64) - o_ref)
    bound = gate.plain_bound(o_ref, rtol, atol)
    assert (err <= bound).all(), f"{tag}: O err/bound {float((err / bound).max()):.3f}"
    assert (np.abs(lg.astype(np.float64) - L)[any_live] <= rtol * L[any_live]).all(), f"{tag}: l"
    assert (mg.astype(np.float64)[any_live] == m[any_live]).all(), f"{tag}: m is not the maximum"
    if (~any_live).any():   # a row empty in every part: what run_case checks of the forwards
        assert (og[np.broadcast_to(~any_live[:, None, :], og.shape)] == 0).all(), tag
        assert (lg[~any_live] == 0).all(), tag
        assert mg[~any_live].tobytes() == b"\xfa" * (mg[~any_live].size * np.dtype(dtype).itemsize), tag


NQS = (1, 7, 33, 130, 136)   # 136: a multiple of every vector width (the vector path); the others: scalar + tail


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_merge_kernel_sweep(dtype, n):
    for nq in NQS:
        for v_d in (1, 8, 72):    # below, at and past one chunk of channel rows
            for b in (1, 3):
                Os, ls, ms = synthetic_partials(dtype, n, b, v_d, nq, seed=nq * 1000 + v_d * 10 + b + n)
                if nq >= 7:
                    _, _, _, any_live = merge_reference(Os, ls, ms)
                    assert (~any_live).any() and any_live.any()
                check_merge(dtype, Os, ls, ms, call_merge(dtype, Os, ls, ms), f"n={n} nq={nq} v_d={v_d} b={b}")


MERGE_SLAB = 65535   # fa_merge_partials launches at most this many slices at once: the grid's y extent


@pytest.mark.parametrize("nq", [7, 8], ids=["scalar", "vector"])
@pytest.mark.parametrize("b", [MERGE_SLAB, MERGE_SLAB + 1, 2 * MERGE_SLAB + 1], ids=["one_slab", "plus_one", "three_slabs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_merge_kernel_large_batch(dtype, b, nq):
    """The slab loop of fa_merge_partials at its real limit: one slab exactly, one slab and one slice, three slabs,
    every slice against the float64 reference.  nq = 7 takes the scalar path; with nq = 8 every slab's offset is
    a multiple of 16 bytes in every dtype, so the later slabs stay on the vector path.  Rows that are empty in
    every part lie in every slab."""
    Os, ls, ms = synthetic_partials(dtype, 3, b, 4, nq, seed=b % 1000 + nq)
    any_live = np.any([x != 0 for x in ls], axis=0)
    for b0 in range(0, b, MERGE_SLAB):
        slab = any_live[b0:b0 + MERGE_SLAB]
        assert (~slab).any() and slab.any(), b0
    check_merge(dtype, Os, ls, ms, call_merge(dtype, Os, ls, ms), f"b={b} nq={nq}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_merge_kernel_misaligned(dtype):
    """Every tensor, inputs and outputs, one element off 16-byte alignment (nq a multiple of the vector width)."""
    Os, ls, ms = synthetic_partials(dtype, 3, 3, 9, 136, seed=5)
    got = call_merge(dtype, Os, ls, ms, misalign=True)
    check_merge(dtype, Os, ls, ms, got, "misaligned")
    for a, b_ in zip(got, call_merge(dtype, Os, ls, ms)):
        assert a.tobytes() == b_.tobytes()   # the scalar and the vector path agree bit for bit


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_merge_kernel_underflow_and_equal_m(dtype):
    """One part's m sits 100 below another's: its weight underflows to 0 (fp16, fp32) and the result is that
    of the other parts alone, finite.  And equal m in every part."""
    Os, ls, ms = synthetic_partials(dtype, 3, 2, 9, 136, seed=11, empty=False)
    ms[0] = np.full_like(ms[0], 30.0)
    ms[1] = np.full_like(ms[1], 29.0)
    ms[2] = np.full_like(ms[2], -70.0)
    got = call_merge(dtype, Os, ls, ms)
    check_merge(dtype, Os, ls, ms, got, "underflow")
    o_two, _, _, _ = merge_reference(Os[:2], ls[:2], ms[:2])
    rtol, atol = TOL[dtype]["fwd"]
    assert (np.abs(got[0].astype(np.float64) - o_two) <= gate.plain_bound(o_two, rtol, atol)).all()
    ms = [np.full_like(x, -3.5) for x in ms]
    check_merge(dtype, Os, ls, ms, call_merge(dtype, Os, ls, ms), "equal m")


@pytest.mark.parametrize("nq", [33, 136])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_merge_kernel_bitwise_properties(dtype, nq):
    same = lambda x, y: all(a.tobytes() == b_.tobytes() for a, b_ in zip(x, y))  # noqa: E731
    # one part comes back bit for bit (a negative zero in O included)
    Os, ls, ms = synthetic_partials(dtype, 1, 2, 9, nq, seed=21)
    ls[0][0, 1], ms[0][0, 1], Os[0][0, 0, 1] = 3.0, 1.5, -0.0
    assert np.signbit(Os[0][0, 0, 1])
    assert same(call_merge(dtype, Os, ls, ms), (Os[0], ls[0], ms[0]))
    # a part that is empty in every row changes nothing, wherever it stands
    Os, ls, ms = synthetic_partials(dtype, 2, 3, 9, nq, seed=22)
    base = call_merge(dtype, Os, ls, ms)
    Oe, le, me = (np.zeros_like(x) for x in (Os[0], ls[0], ms[0]))
    make_empty(Oe, le, me, np.ones(le.shape, dtype=bool))
    for pos in (0, 1, 2):
        ins = lambda xs, e: xs[:pos] + [e] + xs[pos:]  # noqa: E731
        assert same(call_merge(dtype, ins(Os, Oe), ins(ls, le), ins(ms, me)), base), pos
    # deterministic
    assert same(call_merge(dtype, Os, ls, ms), base)
    # a slice's bits do not depend on b
    one = call_merge(dtype, [x[1:2] for x in Os], [x[1:2] for x in ls], [x[1:2] for x in ms])
    assert same(one, tuple(x[1:2] for x in base))


def test_merge_partials_wrapper_matches_the_entry_point():
    Os, ls, ms = synthetic_partials(np.float16, 3, 2, 8, 136, seed=31)
    got = fa.merge_partials(*([_to_dev(x) for x in xs] for xs in (Os, ls, ms)))
    torch.cuda.synchronize()
    for a, b_ in zip(got, call_merge(np.float16, Os, ls, ms)):
        assert a.cpu().numpy().tobytes() == b_.tobytes()
    # 2d: batch (1, 2), sequence (8, 17)
    r = lambda x, ch: x.reshape((1, 2) + ((ch,) if ch else ()) + (8, 17))  # noqa: E731
    got2 = fa.merge_partials([_to_dev(r(x, 8)) for x in Os], [_to_dev(r(x, 0)) for x in ls],
                             [_to_dev(r(x, 0)) for x in ms], seq_dims=2)
    assert got2[0].shape == (1, 2, 8, 8, 17) and got2[1].shape == (1, 2, 8, 17)
    for a, b_ in zip(got2, got):
        assert torch.equal(a.reshape(b_.shape), b_)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_accumulate_parts(dtype, n):
    """out = T(sum in part order, accumulated in fp32 / fp64): within one rounding of T of the exact sum, plus
    the n - 1 roundings of the accumulator (u_acc each, of at most sum |in_i|)."""
    u_t, u_acc = U_ROUND[dtype]
    L = _lib.lib()
    for count in NQS + (2048 + 5,):
        for misalign in (False, True):
            rng = np.random.default_rng(count * 10 + n)
            parts = [rng.uniform(-2, 2, count).astype(dtype) for _ in range(n)]
            dparts = [_to_dev(x, misalign) for x in parts]
            out = _empty_like(parts[0], misalign)
            st = L.fa_accumulate_parts(torch.cuda.current_stream(_dev()).cuda_stream, DT_ID[dtype], count, n,
                                       _lib.pointer_array([t.data_ptr() for t in dparts]), out.data_ptr())
            assert st == _lib.FA_OK, _lib.last_error()
            torch.cuda.synchronize()
            exact = np.sum([x.astype(np.float64) for x in parts], axis=0)
            mag = np.sum([np.abs(x.astype(np.float64)) for x in parts], axis=0)
            err = np.abs(out.cpu().numpy().astype(np.float64) - exact)
            tiny = float(np.finfo(dtype).smallest_subnormal) / 2   # a result below T's normal range
            assert (err <= u_t * np.abs(exact) + tiny + (1 + u_t) * (n - 1) * u_acc * mag).all(), (count, misalign)
            if n == 1:
                assert out.cpu().numpy().tobytes() == parts[0].tobytes()


# ------------------------------------------------------------------------------------------------
# combined attention, forward and backward
# ------------------------------------------------------------------------------------------------
class Spec:
    """One part of a case: the policy and its arguments, and the key sequence shape."""

    def __init__(self, policy, ks, sync_mode="none_front", window_size=1, log2_stride_size=0, is_causal=False):
        self.policy, self.ks, self.sync_mode = policy, tuple(ks), sync_mode
        self.ws, self.ls, self.causal = window_size, log2_stride_size, is_causal

    def problem(self, seq_dims):
        return O.Problem(self.policy, seq_dims, self.sync_mode, self.ws, self.ls, self.causal)


CASES = {
    # name: (dtype, seq_dims, qs, d, v_d, parts)
    "window_global_f16": (np.float16, 1, (200,), 64, 64, [Spec("local", (200,), window_size=33), Spec("full", (8,))]),
    "window_global_f32": (np.float32, 1, (200,), 32, 40, [Spec("local", (200,), window_size=33), Spec("full", (8,))]),
    "window_global_f64": (np.float64, 1, (200,), 16, 16, [Spec("local", (200,), window_size=33), Spec("full", (8,))]),
    "causal_sinks_f16": (np.float16, 1, (130,), 128, 128, [Spec("causal", (130,)), Spec("full", (4,))]),
    "causal_sinks_f32": (np.float32, 1, (130,), 32, 32, [Spec("causal", (130,)), Spec("full", (4,))]),
    "window2d_prompt_f16": (np.float16, 2, (12, 10), 64, 64,
                            [Spec("local", (12, 10), window_size=3), Spec("full", (1, 8))]),
    "key_shards_f16": (np.float16, 1, (77,), 64, 64, [Spec("full", (100,)), Spec("full", (64,)), Spec("full", (37,))]),
    "key_shards_f32": (np.float32, 1, (77,), 32, 32, [Spec("full", (100,)), Spec("full", (64,)), Spec("full", (37,))]),
    # two strided windows.  Under none_front a causal window over as many keys as queries always holds the
    # query's own position, so no row could be empty in both parts; the first window therefore strides over
    # 24 keys under scale_front (key k at position 4k, stride 4: only queries at multiples of 4 see a key),
    # the second over 48 keys (key k at position 2k, stride 2: only even queries).  Odd queries are empty in
    # both parts, queries = 2 mod 4 in the first only.
    "empty_rows_f16": (np.float16, 1, (96,), 32, 32,
                       [Spec("local", (24,), "scale_front", window_size=4, log2_stride_size=2, is_causal=True),
                        Spec("local", (48,), "scale_front", window_size=3, log2_stride_size=1)]),
    "empty_rows_f32": (np.float32, 1, (96,), 16, 24,
                       [Spec("local", (24,), "scale_front", window_size=4, log2_stride_size=2, is_causal=True),
                        Spec("local", (48,), "scale_front", window_size=3, log2_stride_size=1)]),
    # the split paths: 16 global keys against 2300 queries take the backward's query-chunk plan; 33 queries
    # against 2100 keys take the split-key forward and the backward's key-chunk dQ plan
    "split_q_f16": (np.float16, 1, (2300,), 64, 64, [Spec("local", (2300,), window_size=33), Spec("full", (16,))]),
    "split_k_f16": (np.float16, 1, (33,), 64, 64, [Spec("full", (2100,)), Spec("local", (33,), window_size=5)]),
    # two key shards over 65538 slices: the merge runs a second slab (MERGE_SLAB slices and 3 more)
    "many_slices_f16": (np.float16, 1, (8,), 8, 8, [Spec("full", (8,)), Spec("full", (8,))]),
    "many_slices_f32": (np.float32, 1, (8,), 8, 8, [Spec("full", (8,)), Spec("full", (8,))]),
}
BATCH = (1, 2)
# cases with a batch of their own, checked on a fixed sample of its slices: name -> (batch, slices); here the first
# and the last slices of both slabs of the merge, and a few more
SAMPLED = {name: ((65538,), (0, 1, 2, 32767, 32768, 40000, 65533, 65534, 65535, 65536, 65537))
           for name in ("many_slices_f16", "many_slices_f32")}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs (U(-2, 2), as run_case) and the dense float64 reference of a case, computed once and shared.  A
    SAMPLED case keeps its whole inputs under "device" (what runs) and "slices"; everything else, inputs and
    reference, is of those slices only, as a case of that many slices."""
    dtype, seq_dims, qs, d, v_d, specs = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    batch, slices = SAMPLED.get(name, (BATCH, None))
    nq = int(np.prod(qs))
    Q = rng.uniform(-2, 2, batch + (d,) + qs).astype(dtype)
    Ks = [rng.uniform(-2, 2, batch + (d,) + s.ks).astype(dtype) for s in specs]
    Vs = [rng.uniform(-2, 2, batch + (v_d,) + s.ks).astype(dtype) for s in specs]
    dO = rng.uniform(-2, 2, batch + (v_d,) + qs).astype(dtype)
    device = dict(Q=Q, Ks=Ks, Vs=Vs, dO=dO)
    if slices is not None:
        pick = lambda x: x[list(slices)]  # noqa: E731  (one batch axis)
        Q, Ks, Vs, dO = pick(Q), [pick(x) for x in Ks], [pick(x) for x in Vs], pick(dO)
    b = int(np.prod(Q.shape[:len(batch)]))
    masks = [O.problem_mask(s.problem(seq_dims), qs, s.ks) for s in specs]
    mask = np.concatenate(masks, axis=1)
    nks = [int(np.prod(s.ks)) for s in specs]
    q = Q.reshape(b, d, nq).astype(np.float64)
    k = np.concatenate([x.reshape(b, d, n) for x, n in zip(Ks, nks)], axis=2).astype(np.float64)
    v = np.concatenate([x.reshape(b, v_d, n) for x, n in zip(Vs, nks)], axis=2).astype(np.float64)
    do = dO.reshape(b, v_d, nq).astype(np.float64)
    scale = 1.0 / math.sqrt(d)
    ha = mask.any(axis=1)
    o_ref = np.zeros((b, v_d, nq)); dq = np.zeros((b, d, nq)); dk = np.zeros_like(k); dv = np.zeros_like(v)
    edges = np.cumsum([0] + nks)
    dq_part_max = np.zeros(len(specs))
    for i in range(b):
        s = np.where(mask, (q[i].T @ k[i]) * scale, -np.inf)
        mrow = np.where(ha, s.max(axis=1, initial=-np.inf), 0.0)
        p = np.exp(s - mrow[:, None])
        p = p / np.where(ha, p.sum(axis=1), 1.0)[:, None]
        o_ref[i] = v[i] @ p.T
        dv[i] = do[i] @ p
        dp = do[i].T @ v[i]
        D = np.sum(do[i] * o_ref[i], axis=0)
        ds = p * (dp - D[:, None]) * scale
        dq[i] = k[i] @ ds.T
        dk[i] = q[i] @ ds
        for j in range(len(specs)):
            c0, c1 = edges[j], edges[j + 1]
            dq_part_max[j] = max(dq_part_max[j], float(np.abs(k[i][:, c0:c1] @ ds[:, c0:c1].T).max()))
    # L and M of the union from forward_f64's per-part values
    per = [O.forward_f64(Q.reshape((b, d) + qs), K.reshape((b, d) + s.ks), V.reshape((b, v_d) + s.ks),
                         s.problem(seq_dims)) for K, V, s in zip(Ks, Vs, specs)]
    Mi = np.stack([np.where(h[None, :], M.reshape(b, nq), -np.inf) for _, _, M, h in per])
    Li = np.stack([L.reshape(b, nq) for _, L, _, _ in per])
    M = np.where(ha[None, :], Mi.max(axis=0), 0.0)
    L = np.sum(np.where(np.isfinite(Mi), Li * np.exp(np.where(np.isfinite(Mi), Mi, 0.0) - M[None]), 0.0), axis=0)
    assert (np.stack([h for _, _, _, h in per]).any(axis=0) == ha).all()
    return dict(Q=Q, Ks=Ks, Vs=Vs, dO=dO, masks=masks, mask=mask, ha=ha, O=o_ref, L=L, M=M, dQ=dq,
                dKs=[dk[:, :, edges[j]:edges[j + 1]] for j in range(len(specs))],
                dVs=[dv[:, :, edges[j]:edges[j + 1]] for j in range(len(specs))], dq_part_max=dq_part_max,
                kcat=k, vmax=float(np.abs(v).max()), b=b, nq=nq, device=device, slices=slices)


def o_bound(name):
    dtype = CASES[name][0]
    c = case_data(name)
    rtol, atol = TOL[dtype]["fwd"]
    return gate.plain_bound(c["O"], rtol, atol) + U_ROUND[dtype][0] * c["vmax"]


def grad_bounds(name):
    """{gradient: bound}; dKs / dVs are lists over the parts."""
    dtype, _, _, _, _, specs = CASES[name]
    c = case_data(name)
    rtol, atol = TOL[dtype]["bwd"]
    return dict(dQ=gate.plain_bound(c["dQ"], rtol, atol) + len(specs) * U_ROUND[dtype][0] * float(c["dq_part_max"].max()),
                dKs=[gate.plain_bound(x, rtol, atol) for x in c["dKs"]],
                dVs=[gate.plain_bound(x, rtol, atol) for x in c["dVs"]])


def check_l_m(name, l, m):
    """run_case's checks of l and m (tests/test_gpu_parity.py), against the union's L and M."""
    dtype, _, _, d, _, _ = CASES[name]
    c = case_data(name)
    check_l_m_values(dtype, d, c["Q"].reshape(c["b"], d, c["nq"]), c["kcat"], c["mask"], c["ha"], c["L"], c["M"], l, m)


def check_l_m_values(dtype, d, Q, kcat, mask, ha, L, M, l, m, offset_scores=False):
    """check_l_m on explicit values (tests/test_gpu_union_fuzz.py shares it): Q [b, d, nq], the concatenated keys
    kcat [b, d, nk], the union's mask [nq, nk], its non-empty rows ha and float64 L, M [b, nq] against the stored
    l and m.  Returns the worst error / tolerance of m and of l.

    offset_scores (the sweep's inputs only; check_l_m never sets it): fp16 scores that carry an offset of up to 12
    in one channel.  The rounding of the pre-scaled Q that m's tolerance allows every score, (2^-11 + d 2^-24) of
    sum_c |q_c k_c| / sqrt(d), is then coherent over a part's keys (one product carries it) and smaller than the step
    of the stored m: l, the sum of exp(s - stored m), moves by that factor while the stored m stays where it
    is, so l gets exp(that term) - 1 relative beside its own tolerance.  Sweep seed 4 (fp16, d = 64, a 16-key part
    12 above the others): fp16(2 log2(e) / 8) is 2.1e-4 low, every score of that part 2.5e-3 low, and l 0.25 % low in
    every row, 1.32 x its un-extended tolerance at the worst one (22 of the sweep's 240 default cases exceed it, all
    fp16 with an offset of 6 or 12, the worst 2.47 x at seed 21); U(-2, 2) inputs keep the same effect at 6e-4."""
    b, _, nq = Q.shape
    rtol, atol = TOL[dtype]["fwd"]
    lg = l.reshape(b, nq).astype(np.float64)
    mg = m.reshape(b, nq)
    worst = dict(m=0.0, l=0.0, l_plain=0.0)
    if ha.any():
        M64, L64 = M[:, ha], L[:, ha]
        m_f = mg[:, ha].astype(np.float64)
        ulp = np.abs(np.spacing(np.abs(M64).astype(dtype))).astype(np.float64)
        eps = float(np.finfo(dtype).eps)
        Qf = Q.astype(np.float64)
        if dtype == np.float16:
            rowdot = gate.max_abs_dot(Qf, kcat, mask)[:, ha] / math.sqrt(d)
            m_tol = 2 * ulp + np.maximum(1e-3 * np.maximum(np.abs(M64), 1.0),
                                         (2.0 ** -11 + d * 2.0 ** -24) * rowdot + 4.9e-4)
            score_rounding = (2.0 ** -11 + d * 2.0 ** -24) * rowdot
        else:
            dot_bound = np.abs(Qf).sum(axis=1)[:, ha] * max(float(np.abs(kcat).max()), 1e-30) / math.sqrt(d)
            m_tol = 2 * ulp + 1e-6 * np.abs(M64) + np.maximum(1e-6 if dtype != np.float64 else 1e-12, 2 * eps * dot_bound)
        assert np.isfinite(m_f).all() and np.isfinite(lg[:, ha]).all(), "l or m is not finite"
        assert (np.abs(m_f - M64) <= m_tol).all(), f"m: max err {np.abs(m_f - M64).max():.3e}"
        l_ref = L64 * np.exp(M64 - m_f)    # relative to the stored m
        l_rtol = max(rtol, 1e-6 if dtype == np.float16 else rtol)
        scale = max(float(np.abs(l_ref).max()), 1.0)
        l_tol = atol * scale + l_rtol * np.abs(l_ref)
        l_plain = float((np.abs(lg[:, ha] - l_ref) / l_tol).max())
        if offset_scores and dtype == np.float16:
            l_tol = l_tol + np.expm1(score_rounding) * np.abs(l_ref)
        assert (np.abs(lg[:, ha] - l_ref) <= l_tol).all(), f"l: max err / tolerance {float((np.abs(lg[:, ha] - l_ref) / l_tol).max()):.3f}"
        worst = dict(m=float((np.abs(m_f - M64) / m_tol).max()), l=float((np.abs(lg[:, ha] - l_ref) / l_tol).max()), l_plain=l_plain)
    if (~ha).any():
        assert (lg[:, ~ha] == 0).all()
        assert mg[:, ~ha].tobytes() == b"\xfa" * (mg[:, ~ha].size * np.dtype(dtype).itemsize)
    return worst


def run_combined(name):
    """The case through combined_1d / combined_2d, forward and backward; numpy results."""
    dtype, seq_dims, qs, d, v_d, specs = CASES[name]
    c = case_data(name)
    dev = c["device"]
    tq = _to_dev(dev["Q"]).requires_grad_(True)
    tks = [_to_dev(x).requires_grad_(True) for x in dev["Ks"]]
    tvs = [_to_dev(x).requires_grad_(True) for x in dev["Vs"]]
    parts = [fa.Part(s.policy, tk, tv, s.sync_mode, s.ws, s.ls, s.causal) for s, tk, tv in zip(specs, tks, tvs)]
    o, l, m = (fa.combined_1d if seq_dims == 1 else fa.combined_2d)(tq, parts, returning_l_m=True)
    assert not l.requires_grad and not m.requires_grad
    o.backward(_to_dev(dev["dO"]))
    torch.cuda.synchronize()
    pick = sampler(name)
    flat = lambda t, ch: pick(t.detach().cpu().numpy()).reshape(c["b"], ch, -1)  # noqa: E731
    return dict(O=flat(o, v_d), l=pick(l.cpu().numpy()), m=pick(m.cpu().numpy()), dQ=flat(tq.grad, d),
                dKs=[flat(t.grad, d) for t in tks], dVs=[flat(t.grad, v_d) for t in tvs])


def sampler(name):
    """What takes a result of the case's whole batch to the slices that case_data holds."""
    slices = case_data(name)["slices"]
    return (lambda x: x) if slices is None else (lambda x: x[list(slices)])


def ratio(got, ref, bound):
    got = got.astype(np.float64)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


def check_combined(name, got):
    dtype = CASES[name][0]
    c = case_data(name)
    ha = c["ha"]
    ratios = {"O": ratio(got["O"], c["O"], o_bound(name))}
    gb = grad_bounds(name)
    ratios["dQ"] = ratio(got["dQ"], c["dQ"], gb["dQ"])
    for j in range(len(c["Ks"])):
        ratios[f"dK{j}"] = ratio(got["dKs"][j], c["dKs"][j], gb["dKs"][j])
        ratios[f"dV{j}"] = ratio(got["dVs"][j], c["dVs"][j], gb["dVs"][j])
    print(f"combine_gate {name} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    check_l_m(name, got["l"], got["m"])
    if (~ha).any():
        assert (got["O"][:, :, ~ha] == 0).all()


@pytest.mark.parametrize("name", [n for n in sorted(CASES)
                                  if not n.startswith(("key_shards", "empty_rows", "split", "many_slices"))])
def test_combined(name):
    check_combined(name, run_combined(name))


@pytest.mark.parametrize("name", ["key_shards_f16", "key_shards_f32", "many_slices_f16", "many_slices_f32"])
def test_combined_key_shards(name):
    """Three key shards under the full policy against the whole problem, and against full_1d on the unsplit K.
    many_slices: two shards of 8 keys over 65538 slices, forward and backward, so that the merge and every forward
    and backward launcher under combined_1d see a second slab or slice indices past 16 bits; checked on the
    sampled slices."""
    got = run_combined(name)
    check_combined(name, got)
    c = case_data(name)
    dev = c["device"]
    cat = lambda xs: _to_dev(np.concatenate(xs, axis=-1))  # noqa: E731
    whole = fa.full_1d(_to_dev(dev["Q"]), cat(dev["Ks"]), cat(dev["Vs"]))
    torch.cuda.synchronize()
    whole = sampler(name)(whole.cpu().numpy()).reshape(got["O"].shape)
    assert ratio(whole, c["O"], o_bound(name)) <= 1.0   # (full_1d itself, for scale)
    assert ratio(got["O"], whole.astype(np.float64), o_bound(name)) <= 1.0


@pytest.mark.parametrize("name", ["empty_rows_f16", "empty_rows_f32"])
def test_combined_empty_rows(name):
    c = case_data(name)
    rows = np.stack([mk.any(axis=1) for mk in c["masks"]])
    empty_in_all = int((~rows).all(axis=0).sum())
    empty_in_one = int(((~rows).sum(axis=0) == 1).sum())
    assert empty_in_all > 0 and empty_in_one > 0, (empty_in_all, empty_in_one)
    check_combined(name, run_combined(name))


def _plan(fn, dtype, policy, qs, ks, d, v_d, ws=1):
    out = (ctypes.c_int32 * 4)()
    prob = _lib.make_problem(DT_ID[dtype], {"full": _lib.FULL, "local": _lib.LOCAL}[policy], 1, _lib.NONE_FRONT,
                             int(np.prod(BATCH)), qs, ks, d, v_d, ws)
    assert fn(prob, out) == _lib.FA_OK
    return out[0]


def test_combined_split_query_backward():
    """16 global keys against 2300 queries: that part's backward takes fa_backward_split's query-chunk plan,
    fed the merged statistics."""
    L = _lib.lib()
    assert _plan(L.fa_backward_split_q_plan, np.float16, "full", (2300,), (16,), 64, 64) >= 2
    check_combined("split_q_f16", run_combined("split_q_f16"))


def test_combined_split_key_paths():
    """33 queries against 2100 keys: that part's forward goes through fa_forward_ws's split-key path and its
    backward through the key-chunk dQ plan, fed the merged statistics."""
    L = _lib.lib()
    assert _plan(L.fa_forward_split_plan, np.float16, "full", (33,), (2100,), 64, 64) >= 2
    assert _plan(L.fa_backward_split_plan, np.float16, "full", (33,), (2100,), 64, 64) >= 2
    check_combined("split_k_f16", run_combined("split_k_f16"))


def test_user_composition_drops_the_normaliser_gradient():
    """What is possible without the feature: the window + global case composed in torch from
    local_1d(..., returning_l_m=True) and full_1d(..., returning_l_m=True), autograd through O only (l and m
    are non-differentiable).  Its forward passes the bound; its dK of the global keys does not: the gradient
    through each part's normaliser is dropped.  Pins what combined_1d fixes, and that the bound sees it."""
    name = "window_global_f16"
    c = case_data(name)
    tq = _to_dev(c["Q"]).requires_grad_(True)
    tks = [_to_dev(x).requires_grad_(True) for x in c["Ks"]]
    tvs = [_to_dev(x).requires_grad_(True) for x in c["Vs"]]
    o1, l1, m1 = fa.local_1d(tq, tks[0], tvs[0], 33, 0, False, "none_front", returning_l_m=True)
    o2, l2, m2 = fa.full_1d(tq, tks[1], tvs[1], returning_l_m=True)
    m = torch.maximum(m1, m2).float()
    e1, e2 = l1 * torch.exp(m1.float() - m), l2 * torch.exp(m2.float() - m)
    o = ((e1 / (e1 + e2))[..., None, :] * o1.float() + (e2 / (e1 + e2))[..., None, :] * o2.float()).half()
    o.backward(_to_dev(c["dO"]))
    torch.cuda.synchronize()
    b, nq = c["b"], c["nq"]
    assert ratio(o.detach().cpu().numpy().reshape(b, -1, nq), c["O"], o_bound(name)) <= 1.0
    gb = grad_bounds(name)
    r = ratio(tks[1].grad.cpu().numpy().reshape(c["dKs"][1].shape), c["dKs"][1], gb["dKs"][1])
    print(f"combine_gate user_composition dK1={r:.3f}")
    assert r > 1.0, r


# ------------------------------------------------------------------------------------------------
# a part far above or below the others: the dominance ladder (the inputs and the gate of the sweep,
# tests/test_gpu_union_fuzz.py, on fixed cases)
# ------------------------------------------------------------------------------------------------
def _part(policy, ks, delta=0, mode="none_front", ws=1, ls=0, causal=False):
    return dict(policy=policy, ks=tuple(ks), delta=delta, mode=mode, ws=ws, ls=ls, causal=causal)


LADDER = {
    # name: (dtype, d, v_d, queries, the part that stays at 0, the part that carries the offset)
    "window_global_f16": (np.float16, 64, 64, 200, _part("local", (200,), ws=33), _part("full", (8,))),
    "window_global_f32": (np.float32, 64, 64, 200, _part("local", (200,), ws=33), _part("full", (8,))),
    "causal_sinks_d160_f16": (np.float16, 160, 160, 130, _part("causal", (130,)), _part("full", (4,))),
    "causal_sinks_d288_f16": (np.float16, 288, 288, 40, _part("causal", (40,)), _part("full", (4,))),
}


def ladder_case(name, delta):
    """The case in the sweep's form: its inputs are test_gpu_union_fuzz.build's (channel 0 of Q is 2, of the offset
    part's K delta * sqrt(d) / 2), its gate test_gpu_union_fuzz.check."""
    dtype, d, v_d, nq, base, lifted = LADDER[name]
    return dict(kind="combined", dtype=dtype, seq=1, misalign=False, seed=10_000 + sorted(LADDER).index(name), split="",
                batch=(2,), g=1, hk=1, d=d, vd=v_d, qs=(nq,), parts=[dict(base), dict(lifted, delta=delta)])


@pytest.mark.parametrize("delta", [-12, -6, -3, 3, 6, 12])
@pytest.mark.parametrize("name", sorted(LADDER))
def test_combined_dominance_ladder(name, delta):
    """One part's scores lifted or lowered by delta against the other's: at -12 its backward gets a merged m far
    above its own scores and its P sits in fp16's subnormal range; at +12 it carries nearly the whole mass and the
    other part's does.  Every gradient under the gate with tests/union_ref.py's scales.  At +-3 the same case with
    every part's gradients taken from its own (l_i, m_i) (mutation a of tests/test_union_fuzz_draws.py, computed in
    float64 on the CPU) must fail that gate: the ladder binds."""
    from tests import test_gpu_union_fuzz as F
    c = ladder_case(name, delta)
    p = F.build(c)
    ref = F.reference(c, p)
    res = F.check(c, ref, F._call(c, p))
    print(f"combine_ladder {name} {delta:+d} " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
    if abs(delta) == 3:
        from tests import test_union_fuzz_draws as UD
        assert UD.applies(c, "a")
        with pytest.raises(AssertionError):
            F.check(c, ref, UD.mutated(c, p, ref, "a"))


# ------------------------------------------------------------------------------------------------
# autograd plumbing of combined_1d
# ------------------------------------------------------------------------------------------------
PLUMBING = [Spec("full", (100,)), Spec("causal", (64,), "scale_end"), Spec("local", (37,), "scale_front", window_size=5)]


def _plumbing_inputs(dtype=np.float16, d=64, v_d=40, nq=77):
    rng = np.random.default_rng(77)
    u = lambda *s: rng.uniform(-2, 2, s).astype(dtype)  # noqa: E731
    return u(2, d, nq), [u(2, d, *s.ks) for s in PLUMBING], [u(2, v_d, *s.ks) for s in PLUMBING], u(2, v_d, nq)


def _combined_grads(Q, Ks, Vs, dO, want, wrap=lambda x: _to_dev(x)):
    """combined_1d over PLUMBING with requires_grad on the tensors named in ``want`` ("Q", "K1", "V2", ...);
    returns (O, l, m, {name: gradient or None}) as bytes-comparable numpy."""
    leaves = {"Q": wrap(Q), **{f"K{j}": wrap(x) for j, x in enumerate(Ks)}, **{f"V{j}": wrap(x) for j, x in enumerate(Vs)}}
    for k in want:
        leaves[k].requires_grad_(True)
    parts = [fa.Part(s.policy, leaves[f"K{j}"], leaves[f"V{j}"], s.sync_mode, s.ws, s.ls, s.causal) for j, s in enumerate(PLUMBING)]
    o, l, m = fa.combined_1d(leaves["Q"], parts, returning_l_m=True)
    if want:
        o.backward(_to_dev(dO))
    torch.cuda.synchronize()
    grads = {k: (None if t.grad is None else t.grad.cpu().numpy()) for k, t in leaves.items()}
    return o.detach().cpu().numpy(), l.cpu().numpy(), m.cpu().numpy(), grads


ALL_LEAVES = ("Q", "K0", "V0", "K1", "V1", "K2", "V2")


@pytest.mark.parametrize("want", [("Q",), ("K1",), ("V2",), ALL_LEAVES[1:]], ids=["Q", "K1", "V2", "all_but_Q"])
def test_combined_gradient_subsets(want):
    """_CombinedFn.backward runs or skips a part by needs_input_grad: whatever is asked for is bit for bit the
    gradient of the run that asks for everything, and nothing else comes back."""
    inputs = _plumbing_inputs()
    full = _combined_grads(*inputs, ALL_LEAVES)
    assert all(full[3][k] is not None and np.abs(full[3][k].astype(np.float64)).max() > 0 for k in ALL_LEAVES)
    sub = _combined_grads(*inputs, want)
    for a, b_ in zip(full[:3], sub[:3]):
        assert a.tobytes() == b_.tobytes()
    for k in ALL_LEAVES:
        if k in want:
            assert sub[3][k] is not None and sub[3][k].tobytes() == full[3][k].tobytes(), k
        else:
            assert sub[3][k] is None, k


def _strided(x):
    """x's values as a non-contiguous device view: every second element of a buffer twice as long in the last axis"""
    buf = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=torch.from_numpy(x).dtype, device=_dev())
    buf[..., ::2] = torch.from_numpy(x).to(_dev())
    view = buf[..., ::2]
    assert not view.is_contiguous() or view.numel() <= 1
    return view


def test_combined_non_contiguous_inputs():
    """Q, every K and every V as strided views: forward and gradients are bit for bit those of the contiguous call."""
    inputs = _plumbing_inputs()
    ref = _combined_grads(*inputs, ALL_LEAVES)
    got = _combined_grads(*inputs, ALL_LEAVES, wrap=_strided)
    for a, b_ in zip(ref[:3], got[:3]):
        assert a.tobytes() == b_.tobytes()
    for k in ALL_LEAVES:
        assert got[3][k].shape == ref[3][k].shape and got[3][k].tobytes() == ref[3][k].tobytes(), k


@pytest.mark.parametrize("policy", ["full", "causal", "local"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=_id)
def test_combined_of_one_part_is_the_plain_wrapper(dtype, policy):
    """One part: the merge hands (O, l, m) back bit for bit, fa_accumulate_parts is skipped, and the backward gets the
    statistics its own forward produced: everything equals full_1d / causal_1d / local_1d bitwise."""
    rng = np.random.default_rng(5)
    u = lambda *s: rng.uniform(-2, 2, s).astype(dtype)  # noqa: E731
    Q, K, V, dO = u(2, 48, 150), u(2, 48, 90), u(2, 40, 90), u(2, 40, 150)
    outs = []
    for combined in (True, False):
        tq, tk, tv = (_to_dev(x).requires_grad_(True) for x in (Q, K, V))
        if combined:
            rule = (9, 1, True) if policy == "local" else ()
            res = fa.combined_1d(tq, [fa.Part(policy, tk, tv, "scale_end", *rule)], returning_l_m=True)
        elif policy == "full":
            res = fa.full_1d(tq, tk, tv, "scale_end", returning_l_m=True)
        elif policy == "causal":
            res = fa.causal_1d(tq, tk, tv, "scale_end", returning_l_m=True)
        else:
            res = fa.local_1d(tq, tk, tv, 9, 1, True, "scale_end", returning_l_m=True)
        res[0].backward(_to_dev(dO))
        torch.cuda.synchronize()
        outs.append([t.detach().cpu().numpy() for t in res] + [t.grad.cpu().numpy() for t in (tq, tk, tv)])
    for name, a, b_ in zip(("O", "l", "m", "dQ", "dK", "dV"), *outs):
        assert a.tobytes() == b_.tobytes(), name
