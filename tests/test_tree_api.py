"""CPU tests of the tree-masked draft interface: the exports, the plan and workspace functions
against the plain twins', the host-side statuses of the four fa_forward_*_tree* entry points with pointers that are
never dereferenced, and the draft_mask keyword's own errors (raised before any device call)."""

import contextlib
import ctypes

import pytest
import torch

from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

HK = 2
FORWARDS = ("fa_forward_ragged_tree", "fa_forward_paged_tree", "fa_forward_ragged_tree_fp8", "fa_forward_paged_tree_fp8")
PLANS = ("fa_forward_ragged_tree_plan", "fa_forward_paged_tree_plan", "fa_forward_ragged_tree_workspace_bytes",
         "fa_forward_paged_tree_workspace_bytes")


def test_exported():
    for name in FORWARDS + PLANS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "tree-masked" in _lib.lib().fa_build_info().decode()
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "fa_api.h")) as f:
        header = f.read()
    for name in FORWARDS + PLANS:
        assert name + "(" in header
    assert "it must be finite" in header and "const uint32_t* draft_mask" in header


def test_the_entry_point_names_follow_the_one_rule():
    assert "tree" in _lib.DECODE_FORMS
    assert _lib.decode_entry_points("ragged", "tree", True) == (
        "fa_forward_ragged_tree_plan", "fa_forward_ragged_tree_workspace_bytes", "fa_forward_ragged_tree_fp8")
    assert _lib.decode_entry_points("paged", "tree", False) == (
        "fa_forward_paged_tree_plan", "fa_forward_paged_tree_workspace_bytes", "fa_forward_paged_tree")
    for cache in _lib.DECODE_CACHES:
        for fp8 in (False, True):
            twin = getattr(_lib.lib(), _lib.decode_entry_points(cache, "plain", fp8)[2]).argtypes
            tree = getattr(_lib.lib(), _lib.decode_entry_points(cache, "tree", fp8)[2]).argtypes
            assert len(tree) == len(twin)
            moved = [i for i, (a, b) in enumerate(zip(twin, tree)) if a is not b]
            assert moved == [len(twin) - 6] and tree[moved[0]] is ctypes.c_void_p  # (the mask where tail_causal stood)


def test_the_docstrings_state_the_rule_and_the_contract():
    for doc in (fa.ragged_1d.__doc__, fa.paged_1d.__doc__):
        assert "draft_mask" in doc and "tail_causal=True" in doc and "overwritten in place" in doc
    assert "must be finite" in fa.ragged_1d.__doc__ and "bits at or past Nq are ignored" in fa.ragged_1d.__doc__


# ------------------------------------------------------------------ the plan and the workspace are the twins'
def _prob(nq=4, cap=2048, d=64, g=4, b=None, policy=_lib.FULL, dtype=_lib.F16, vd=None):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, 2 * g if b is None else b, (nq,), (cap,), d,
                             d if vd is None else vd)


SHAPES = [dict(nq=1, g=1), dict(nq=5, g=1), dict(nq=33, g=1), dict(nq=64, g=1), dict(nq=128, g=1, cap=2112),
          dict(nq=16, g=4), dict(nq=7, g=8), dict(nq=16, g=8, d=128), dict(nq=4, g=4, d=40, vd=72, cap=1536),
          dict(nq=129, g=1), dict(nq=64, g=4), dict(d=129, g=4), dict(dtype=_lib.F32, g=4), dict(nq=8, g=8, cap=192)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_the_plans_and_workspaces_are_the_plain_twins(shape):
    L = _lib.lib()
    g = shape["g"]
    p = _prob(**shape)
    for page in (None, 64, 192, 32):
        own = (p, g) + (() if page is None else (page,))
        cache = "ragged" if page is None else "paged"
        if page is not None and int(p.k_seq[0]) % page:
            continue
        a, b = (ctypes.c_int32 * 8)(*([-7] * 8)), (ctypes.c_int32 * 8)(*([-7] * 8))
        st = getattr(L, f"fa_forward_{cache}_tree_plan")(*own, a), getattr(L, f"fa_forward_{cache}_plan")(*own, b)
        assert st[0] == st[1] == _lib.FA_OK and list(a) == list(b)
        need = getattr(L, f"fa_forward_{cache}_tree_workspace_bytes")(*own)
        assert need == getattr(L, f"fa_forward_{cache}_workspace_bytes")(*own) and (need > 0) == (a[0] > 0)
    assert L.fa_forward_ragged_tree_plan(p, g, None) == _lib.FA_ERR_INVALID_ARGUMENT
    assert L.fa_forward_paged_tree_plan(p, g, 64, None) == _lib.FA_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ the ABI's host-side statuses
PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _launch_ragged(p, g, fp8=False, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR, mask=PTR):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_ragged_tree_workspace_bytes(p, g)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_ragged_tree_fp8(None, p, g, None, PTR, PTR, None, None, k_lens, kv_per_len, mask, None,
                                            None, None, ws, ws_bytes)
    return L.fa_forward_ragged_tree(None, p, g, None, PTR, PTR, k_lens, kv_per_len, mask, None, None, None, ws, ws_bytes)


def _launch_paged(p, g, page=64, max_pages=32, fp8=False, num_pages=8, kv_per_len=1, ws=PTR, ws_bytes=None,
                  k_lens=PTR, table=PTR, pools=(PTR, PTR), mask=PTR):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_paged_tree_workspace_bytes(p, g, page)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_paged_tree_fp8(None, p, g, None, pools[0], pools[1], None, None, table, max_pages, page,
                                           num_pages, k_lens, kv_per_len, mask, None, None, None, ws, ws_bytes)
    return L.fa_forward_paged_tree(None, p, g, None, pools[0], pools[1], table, max_pages, page, num_pages, k_lens,
                                   kv_per_len, mask, None, None, None, ws, ws_bytes)


FORMS = [(_launch_ragged, False), (_launch_ragged, True), (_launch_paged, False), (_launch_paged, True)]
FORM_IDS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
def test_a_null_mask_is_an_argument_error_with_text(launch, fp8):
    assert launch(_prob(), 4, fp8=fp8, mask=None) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "draft_mask" in _lib.last_error()
    # an empty batch needs no pointer, the mask included
    kw = dict(k_lens=None) if launch is _launch_ragged else dict(k_lens=None, table=None, pools=(None, None))
    assert launch(_prob(b=0), 4, fp8=fp8, mask=None, **kw) == _lib.FA_OK


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
def test_the_twins_statuses(launch, fp8):
    p = _prob()
    need = int(_lib.lib().fa_forward_ragged_tree_workspace_bytes(p, 4))
    assert need > 0
    # a short or null workspace: nothing is launched (no pointer here could be dereferenced)
    assert launch(p, 4, fp8=fp8, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "workspace_bytes" in _lib.last_error()
    assert launch(p, 4, fp8=fp8, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    # outside the envelope: 129 queries, 256 folded rows, 129 channels, another dtype
    for q in (_prob(nq=129, g=1, b=2), _prob(nq=64, g=4), _prob(d=129), _prob(d=64, vd=129), _prob(dtype=_lib.F32)):
        g = 1 if int(q.q_seq[0]) == 129 else 4
        assert launch(q, g, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
        assert "envelope" in _lib.last_error()
    # the twins' argument errors
    for st in (launch(_prob(policy=_lib.CAUSAL), 4, fp8=fp8, ws_bytes=1 << 30), launch(p, 3, fp8=fp8, ws_bytes=1 << 30),
               launch(p, 4, fp8=fp8, kv_per_len=0), launch(p, 4, fp8=fp8, kv_per_len=3), launch(p, 4, fp8=fp8, k_lens=None)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_the_paged_forms_own_errors(fp8):
    p = _prob()
    assert _launch_paged(p, 4, page=32, max_pages=64, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    assert "page % 64" in _lib.last_error()
    for st in (_launch_paged(p, 4, page=0, fp8=fp8, ws_bytes=1 << 30), _launch_paged(p, 4, max_pages=31, fp8=fp8),
               _launch_paged(p, 4, max_pages=0, fp8=fp8), _launch_paged(p, 4, num_pages=0, fp8=fp8),
               _launch_paged(p, 4, table=None, fp8=fp8), _launch_paged(p, 4, pools=(None, PTR), fp8=fp8)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()


# ------------------------------------------------------------------ the keyword
def _ragged(batch=(3,), hq=8, c=64, cv=64, nq=4, cap=256, kv=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros(batch + (HK, c, cap), dtype=kv),
            torch.zeros(batch + (HK, cv, cap), dtype=kv), torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hq=8, c=64, cv=64, nq=4, page=64, max_pages=4, num_pages=7, kv=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros((num_pages, HK, c, page), dtype=kv),
            torch.zeros((num_pages, HK, cv, page), dtype=kv), torch.zeros(batch + (max_pages,), dtype=torch.int32),
            torch.ones(batch, dtype=torch.int32)]


def _mask(batch=(3,), nq=4, dtype=torch.int32):
    return torch.zeros(batch + (nq, (nq + 31) // 32), dtype=dtype)


CALLS = [(fa.ragged_1d, _ragged), (fa.paged_1d, _paged)]
IDS = ["ragged", "paged"]


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_the_keywords_errors(call, args):
    for bad in (_mask(dtype=torch.int64), _mask(dtype=torch.uint8), _mask(dtype=torch.float32), [[0]], 7):
        with pytest.raises(TypeError, match="draft_mask must be an int32 tensor"):
            call(*args(), tail_causal=True, draft_mask=bad)
    for bad in (_mask(nq=5), _mask(batch=(2,)), _mask(batch=()), torch.zeros((3, 4, 2), dtype=torch.int32),
                torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 1, 4), dtype=torch.int32)):
        with pytest.raises(fa.InvalidArgumentError, match="shape of draft_mask"):
            call(*args(), tail_causal=True, draft_mask=bad)
    with pytest.raises(fa.InvalidArgumentError, match="requires tail_causal=True"):
        call(*args(), draft_mask=_mask())
    with pytest.raises(fa.InvalidArgumentError, match="requires tail_causal=True"):
        call(*args(nq=1), tail_causal=False, draft_mask=_mask(nq=1))
    with pytest.raises(fa.InvalidArgumentError, match="no windowed tree form"):
        call(*args(), tail_causal=True, window_size=16, draft_mask=_mask())
    # a well-formed tree call passes every check but the device check
    for nq in (1, 4, 33):
        with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
            call(*args(nq=nq, hq=2), tail_causal=True, draft_mask=_mask(nq=nq), returning_l_m=True)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(kv=torch.float8_e4m3fn), tail_causal=True, draft_mask=_mask(), k_scale=torch.ones(HK))
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):  # (made contiguous, not refused)
        strided = torch.zeros((3, 2, 33), dtype=torch.int32).transpose(1, 2)
        assert not strided.is_contiguous()
        call(*args(nq=33, hq=2), tail_causal=True, draft_mask=strided)
    # outside the envelope the call raises, as the twins do
    with pytest.raises(NotImplementedError, match="fused envelope"):
        call(*args(c=136), tail_causal=True, draft_mask=_mask())
    with pytest.raises(NotImplementedError, match="fused envelope"):
        call(*args(nq=129, hq=2), tail_causal=True, draft_mask=_mask(nq=129))
    # inference only
    a = args()
    a[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        call(*a, tail_causal=True, draft_mask=_mask())


class _Recorder:
    """Stands in for the library object: every plan is one chunk, every workspace 0 bytes, every forward FA_OK."""

    def __init__(self):
        self.calls, self.args = [], []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            self.args.append(a)
            if name.endswith("_plan"):
                a[-1][0] = 1
            return 0
        return f


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_a_mask_reaches_the_tree_entry_points_with_its_pointer(monkeypatch, call, args, fp8):
    real = _lib.lib()
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(fa, "_check_device_tensors", lambda *t: None)
    monkeypatch.setattr(fa, "_stream_handle", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    cache = "ragged" if call is fa.ragged_1d else "paged"
    a = args(kv=torch.float8_e4m3fn if fp8 else torch.float16)
    mask = _mask()
    out = call(*a, tail_causal=True, draft_mask=mask, returning_l_m=True)
    assert tuple(rec.calls) == fa.decode_entry_points(cache, "tree", fp8)
    assert [len(x) for x in rec.args] == [len(getattr(real, name).argtypes) for name in rec.calls]
    assert rec.args[2][-6] == mask.data_ptr()
    assert out[0].shape == (3, 8, 64, 4) and out[1].shape == out[2].shape == (3, 8, 4)
    # without a mask the call is the plain one
    rec.calls.clear()
    call(*a, tail_causal=True, draft_mask=None)
    assert tuple(rec.calls) == fa.decode_entry_points(cache, "plain", fp8)
