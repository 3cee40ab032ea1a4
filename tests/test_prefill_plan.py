"""CPU tests of the query-blocked plans (fa_forward_ragged_prefill_plan, fa_forward_paged_prefill_plan, the two
workspace functions and the host-side statuses of the four forwards): host-only arithmetic, no
device.  The plan is checked against a model written here from the header's text; by brute force over every length
and block, the chunks below a block's L_b are exactly the chunks that hold a key some query of the block sees."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib

PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _prob(nq, nk, d=64, vd=64, b=None, g=1, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, g if b is None else b, (nq,), (nk,), d, vd)


def _plan(p, g, page=None):
    out = (ctypes.c_int32 * 8)(*([-7] * 8))
    L = _lib.lib()
    st = L.fa_forward_ragged_prefill_plan(p, g, out) if page is None else L.fa_forward_paged_prefill_plan(p, g, page, out)
    assert st == _lib.FA_OK, _lib.last_error()
    return tuple(out)


def _ws(p, g, page=None):
    L = _lib.lib()
    return int(L.fa_forward_ragged_prefill_workspace_bytes(p, g) if page is None else
               L.fa_forward_paged_prefill_workspace_bytes(p, g, page))


def _twin_plan(p, g, page=None):
    out = (ctypes.c_int32 * 6)()
    L = _lib.lib()
    assert (L.fa_forward_ragged_plan(p, g, out) if page is None else L.fa_forward_paged_plan(p, g, page, out)) == 0
    return tuple(out)


def _next_pow2(n):
    return 1 << (n - 1).bit_length()


def _model(g, nq, nk):
    """(chunks, chunk, P_b, rows, nqb) of a blocked call, from include/fa_api.h's text."""
    pb = max(p for p in (1, 2, 4, 8, 16, 32, 64, 128) if g * p <= 128)
    rows, nqb = g * pb, -(-nq // pb)
    kmax = max(1, 64 // nqb)
    min_chunk = 512 if rows <= 64 else 1024
    chunk = max(min_chunk, -(-(-(-nk // 64)) // kmax) * 64)
    return -(-nk // chunk), chunk, pb, rows, nqb


GROUPS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 128)
QUERIES = tuple(range(1, 261)) + (512, 2048)
CAPS = (1, 64, 192, 1100, 2560, 16384, 70000, 1 << 20)


@pytest.mark.parametrize("g", GROUPS)
def test_the_plan_is_the_headers_formula_and_delegates_inside_the_twins_envelope(g):
    seen = set()
    for nk in CAPS:
        for nq in QUERIES:
            p = _prob(nq, nk, g=g)
            plan = _plan(p, g)
            chunks, chunk, pb, rows, nqb = _model(g, nq, nk)
            if g * _next_pow2(nq) <= 128:
                twin = _twin_plan(p, g)
                assert nqb == 1 and twin[0] >= 1
                assert plan == (twin[0], twin[1], pb, rows, 1, 1, 0, 0), (g, nq, nk)
                assert _ws(p, g) == int(_lib.lib().fa_forward_ragged_workspace_bytes(p, g)) > 0
            else:
                assert nqb >= 2 and _twin_plan(p, g)[0] == 0
                assert plan == (chunks, chunk, pb, rows, nqb, 0, 0, 0), (g, nq, nk)
                assert chunk % 64 == 0 and chunks * chunk >= nk > (chunks - 1) * chunk and chunks <= max(1, 64 // nqb)
            seen.add(plan[5])
            if nk % 64 == 0 and nq in (1, 17, 129, 200, 2048):
                assert _plan(p, g, 64) == plan and _ws(p, g, 64) == _ws(p, g)
    assert seen == {0, 1}


@pytest.mark.parametrize("g,nq,nk", [(1, 129, 2600), (1, 300, 1030), (8, 17, 1100), (8, 37, 2560), (16, 20, 2100), (3, 40, 1500),
                                      (128, 2, 1100), (4, 1000, 5000)])
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_the_chunks_below_a_blocks_key_end_are_the_chunks_its_queries_see(g, nq, nk, tail):
    chunks, chunk, pb, rows, nqb, delegated = _plan(_prob(nq, nk, g=g), g)[:6]
    assert delegated == 0 and nqb == -(-nq // pb) >= 2
    most = 0
    for L in range(0, nk + 1):
        for qb in range(nqb):
            q0 = qb * pb
            nq_b = min(pb, nq - q0)
            lb = min(max(L - nq + q0 + nq_b, 0), L) if tail else L
            live = min(chunks, -(-lb // chunk))
            # the keys query q0 + i sees: j <= L - nq + q0 + i (tail), j < L; the union over the block's queries
            newest = min(L - nq + q0 + nq_b - 1, L - 1) if tail else L - 1
            touched = newest // chunk + 1 if newest >= 0 else 0
            assert live == touched, (L, qb)
            # the block-local interval is the twin's: khi = lb - nq_b + i
            if tail and lb > 0 and L - nq + q0 + nq_b <= L:
                assert all(lb - nq_b + i == L - nq + q0 + i for i in (0, nq_b - 1))
            most = max(most, live)
    assert most == chunks  # some length needs every launched chunk


@pytest.mark.parametrize("g,nq,nk,vd", [(1, 129, 2600, 40), (8, 512, 16384, 128), (4, 33, 192, 64), (128, 2, 1100, 72)])
def test_the_workspace_follows_blocks_times_chunks_and_b_does_not_enter_the_plan(g, nq, nk, vd):
    plans = set()
    for bkv in (1, 3, 32):
        p = _prob(nq, nk, vd=vd, b=bkv * g, g=g)
        plan = _plan(p, g)
        plans.add(plan)
        chunks, _, _, rows, nqb, delegated = plan[:6]
        assert delegated == 0
        need = bkv * nqb * chunks * (vd + 3) * rows * 4
        assert _ws(p, g) == -(-need // 256) * 256
    assert len(plans) == 1


def _launch(form, p, g, page=64, max_pages=None, num_pages=8, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR, table=PTR,
            pools=(PTR, PTR)):
    L = _lib.lib()
    paged, fp8 = form.startswith("paged"), form.endswith("fp8")
    if ws_bytes is None:
        ws_bytes = _ws(p, g, page if paged else None)
    sc = (None, None) if fp8 else ()
    if paged:
        max_pages = p.k_seq[0] // page if max_pages is None else max_pages
        fn = L.fa_forward_paged_prefill_fp8 if fp8 else L.fa_forward_paged_prefill
        return fn(None, p, g, None, pools[0], pools[1], *sc, table, max_pages, page, num_pages, k_lens, kv_per_len, 1, None,
                  None, None, ws, ws_bytes)
    fn = L.fa_forward_ragged_prefill_fp8 if fp8 else L.fa_forward_ragged_prefill
    return fn(None, p, g, None, PTR, PTR, *sc, k_lens, kv_per_len, 1, None, None, None, ws, ws_bytes)


FORMS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


@pytest.mark.parametrize("form", FORMS)
def test_outside_the_envelope(form):
    page = 64 if form.startswith("paged") else None
    for p, g in ((_prob(200, 2560, d=136, vd=136, g=2), 2), (_prob(200, 2560, g=2, dtype=_lib.F32), 2),
                 (_prob(2, 2560, b=129, g=129), 129), (_prob(200, 2560, d=64, vd=136, g=2), 2)):
        assert _plan(p, g, page) == (0,) * 8
        assert _ws(p, g, page) == 0
        assert _launch(form, p, g, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
        assert "envelope" in _lib.last_error()
    if page:
        p = _prob(200, 2560, g=2)
        assert _plan(p, 2, 32) == (0,) * 8 and _ws(p, 2, 32) == 0
        assert _launch(form, p, 2, page=32, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
        assert "page % 64" in _lib.last_error()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nq", [4, 200], ids=["delegated", "blocked"])
def test_the_twins_statuses(form, nq):
    g = 4
    p = _prob(nq, 2048, b=2 * g, g=g)
    page = 64 if form.startswith("paged") else None
    need = _ws(p, g, page)
    assert need > 0
    assert _launch(form, p, g, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "workspace_bytes" in _lib.last_error()
    assert _launch(form, p, g, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    # an empty batch needs no pointer
    kw = dict(k_lens=None) if page is None else dict(k_lens=None, table=None, pools=(None, None))
    assert _launch(form, _prob(nq, 2048, b=0, g=g), g, **kw) == _lib.FA_OK
    # the twins' argument errors
    for st in (_launch(form, _prob(nq, 2048, b=2 * g, g=g, policy=_lib.CAUSAL), g, ws_bytes=1 << 30),
               _launch(form, p, 3, ws_bytes=1 << 30), _launch(form, p, g, kv_per_len=0), _launch(form, p, g, kv_per_len=3),
               _launch(form, p, g, k_lens=None)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()
    if page:
        for st in (_launch(form, p, g, page=0, max_pages=32, ws_bytes=1 << 30), _launch(form, p, g, max_pages=31),
                   _launch(form, p, g, max_pages=0), _launch(form, p, g, num_pages=0), _launch(form, p, g, table=None),
                   _launch(form, p, g, pools=(None, PTR)), _launch(form, p, g, page=100, ws_bytes=1 << 30)):
            assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()
    out = (ctypes.c_int32 * 8)()
    L = _lib.lib()
    assert L.fa_forward_ragged_prefill_plan(p, g, None) == _lib.FA_ERR_INVALID_ARGUMENT
    assert L.fa_forward_ragged_prefill_plan(_prob(nq, 2048, b=2 * g, g=g, policy=_lib.CAUSAL), g, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "FA_FULL" in _lib.last_error()
    assert L.fa_forward_paged_prefill_plan(p, g, 100, out) == _lib.FA_ERR_INVALID_ARGUMENT


def test_the_existing_entry_points_keep_their_envelope():
    p = _prob(200, 2048, b=8, g=4)
    assert _twin_plan(p, 4)[0] == 0 and _plan(p, 4)[0] >= 1
    L = _lib.lib()
    st = L.fa_forward_ragged(None, p, 4, None, PTR, PTR, PTR, 1, 1, None, None, None, PTR, 1 << 30)
    assert st == _lib.FA_ERR_UNSUPPORTED and "kv_group * pitch <= 128" in _lib.last_error()
