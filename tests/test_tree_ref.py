"""CPU tests of the tree-masked draft forwards' float64 reference (tests/tree_ref.py) against the ragged reference,
and of draft_mask_from_parents on CPU tensors."""

import numpy as np
import pytest
import torch

from tests import ragged_ref, tree_ref
from tf_flash_attention_amd import flash_attention as fa

CASES = [(1, 1), (1, 5), (2, 33), (4, 16), (1, 64), (1, 128)]  # (g, nq)
CAP = 200


NSEQ, KV_PER_LEN = 3, 2


def _inputs(g, nq, seed, d=8, vd=6, bkv=NSEQ * KV_PER_LEN):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-2, 2, (bkv * g, d, nq))
    K = rng.uniform(-2, 2, (bkv, d, CAP))
    V = rng.uniform(-2, 2, (bkv, vd, CAP))
    return rng, Q, K, V


def _len_sets(nq):
    """Per-slice lengths, NSEQ sequences a set: around 0, nq and a tile, the capacity, and values that are clamped."""
    sets = [[0, nq - 1, nq], [1, nq + 1, 63], [64, 65, CAP], [CAP + 7, -3, nq // 2]]
    return [np.repeat(s, KV_PER_LEN) for s in sets]


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("g,nq", CASES)
def test_the_lower_triangle_is_the_tail_causal_rule(g, nq):
    _, Q, K, V = _inputs(g, nq, 1)
    masks = np.broadcast_to(tree_ref.lower_triangle(nq), (NSEQ, nq, tree_ref.mask_words(nq)))
    for lens in _len_sets(nq):
        _same(tree_ref.forward_f64(Q, K, V, lens, masks, g, KV_PER_LEN),
              ragged_ref.forward_f64(Q, K, V, lens, g, tail_causal=True))


@pytest.mark.parametrize("g,nq", CASES)
def test_an_all_zero_mask_is_the_full_rule_over_the_context(g, nq):
    _, Q, K, V = _inputs(g, nq, 2)
    masks = np.zeros((NSEQ, nq, tree_ref.mask_words(nq)), dtype=np.uint32)
    seen = set()
    for lens in _len_sets(nq):
        ctx = np.maximum(np.clip(lens, 0, CAP) - nq, 0)
        got = tree_ref.forward_f64(Q, K, V, lens, masks, g, KV_PER_LEN)
        _same(got, ragged_ref.forward_f64(Q, K, V, ctx, g))
        for s_kv, c in enumerate(ctx):  # the empty rows where no context is left
            rows = slice(s_kv * g, (s_kv + 1) * g)
            assert (got[3][rows] == (c > 0)).all()
            if c == 0:
                assert not got[0][rows].any() and not got[1][rows].any()
            seen.add(c > 0)
    assert seen == {False, True}


@pytest.mark.parametrize("g,nq", CASES)
def test_garbage_bits_past_nq_change_nothing(g, nq):
    rng, Q, K, V = _inputs(g, nq, 3)
    masks = tree_ref.pack_mask(rng.random((NSEQ, nq, nq)) < 0.5)
    dirty = tree_ref.set_unused_bits(masks, nq)
    assert nq % 32 == 0 or (dirty != masks).any()
    assert (tree_ref.unpack_mask(dirty, nq) == tree_ref.unpack_mask(masks, nq)).all()
    for lens in _len_sets(nq):
        _same(tree_ref.forward_f64(Q, K, V, lens, dirty, g, KV_PER_LEN),
              tree_ref.forward_f64(Q, K, V, lens, masks, g, KV_PER_LEN))


def test_the_rule_slot_by_slot():
    """L < nq: slots at negative positions name no key; L >= nq: slot j is key L - nq + j."""
    nq, cap = 5, 16
    bits = np.zeros((nq, nq), dtype=bool)
    bits[0, 4] = bits[3, 0] = bits[3, 2] = True  # (row 0 sees a LATER slot: a mask is not an interval)
    words = tree_ref.pack_mask(bits)
    m = tree_ref.tree_mask(nq, cap, 3, words)  # base = -2: slots 2, 3, 4 are keys 0, 1, 2
    want = np.zeros((nq, cap), dtype=bool)
    want[0, 2] = want[3, 0] = True
    assert (m == want).all()
    m = tree_ref.tree_mask(nq, cap, 9, words)  # base = 4
    want = np.zeros((nq, cap), dtype=bool)
    want[:, :4] = True
    want[0, 8] = want[3, 4] = want[3, 6] = True
    assert (m == want).all()
    assert not tree_ref.tree_mask(nq, cap, 0, words).any()
    assert (tree_ref.tree_mask(nq, cap, 99, words) == tree_ref.tree_mask(nq, cap, cap, words)).all()


def _parents_cases():
    rng = np.random.default_rng(7)
    out = {}
    for nq in (1, 5, 33, 64, 128):
        out[f"chain{nq}"] = np.arange(nq) - 1
        out[f"star{nq}"] = np.where(np.arange(nq) == 0, -1, 0)
        out[f"forest{nq}"] = np.stack([np.array([rng.integers(-1, i) for i in range(nq)]) for _ in range(3)]).reshape(3, 1, nq)
    return out


@pytest.mark.parametrize("name,parents", list(_parents_cases().items()), ids=list(_parents_cases()))
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_draft_mask_from_parents_is_ancestors_plus_self(name, parents, dtype):
    nq = parents.shape[-1]
    got = fa.draft_mask_from_parents(torch.from_numpy(np.ascontiguousarray(parents)).to(dtype))
    assert got.dtype == torch.int32 and tuple(got.shape) == parents.shape + (tree_ref.mask_words(nq),)
    want = tree_ref.ancestors(parents)
    assert (got.numpy().view(np.uint32) == tree_ref.pack_mask(want)).all()
    if name.startswith("chain"):
        assert (got.numpy().view(np.uint32) == tree_ref.lower_triangle(nq)).all()
    if name.startswith("star"):
        assert want[..., 0].all() and (want.sum(-1) == np.minimum(np.arange(nq) + 1, 2)).all()


def test_draft_mask_from_parents_refuses_other_inputs():
    with pytest.raises(TypeError):
        fa.draft_mask_from_parents([0, 1])
    with pytest.raises(TypeError):
        fa.draft_mask_from_parents(torch.zeros(4))
    with pytest.raises(fa.InvalidArgumentError):
        fa.draft_mask_from_parents(torch.zeros((), dtype=torch.int32))
