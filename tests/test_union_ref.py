"""CPU tests of tests/union_ref.py, the dense float64 reference of the combined / grouped gradient sweep: with one part
it is the oracle (forward_f64, backward_f64, backward_rounding_scale_f64) on that part's problem, for every policy in
1d and 2d and with rows that attend nothing; with two parts it is the inline reference of tests/test_gpu_merge.py; its
grouped helper is the fold and the root-sum-square of tests/test_gpu_grouped.py::test_gradients.

"Equal" is 1e-12 of the tensor's largest element plus 1e-12 relative per element: the oracle walks row chunks and
column bands, so its float64 sums run in another order, and an element that cancels to far below its terms differs in
its last bits by that order alone."""
import numpy as np
import pytest

from oracle import fa_oracle as O
from tests import union_ref
from tests.gate import U_ROUND

CASES = [
    # policy, seq_dims, mode, qs, ks, window, stride, is_causal
    ("full", 1, "none_front", (37,), (50,), 1, 0, False),
    ("causal", 1, "scale_end", (40,), (17,), 1, 0, False),
    ("local", 1, "none_front", (45,), (45,), 7, 0, True),
    ("local", 1, "scale_front", (96,), (24,), 4, 2, True),        # the rows off the stride attend nothing
    ("local", 1, "none_front", (60,), (20,), 5, 0, False),         # the rows past the keys' window attend nothing
    ("full", 2, "none_front", (5, 6), (4, 9), 1, 0, False),
    ("causal", 2, "scale_front", (6, 5), (6, 5), 1, 0, False),
    ("local", 2, "scale_end", (8, 7), (8, 7), 3, 1, False),
    ("local", 2, "none_front", (9, 9), (4, 4), 2, 0, True),        # rows without a key in 2d
]


def _inputs(dtype, b, d, vd, nq, nks, seed):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-2, 2, s).astype(dtype)  # noqa: E731
    return u(b, d, nq), [u(b, d, n) for n in nks], [u(b, vd, n) for n in nks], u(b, vd, nq)


def _same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * max(float(np.abs(b).max()), 1e-300)), \
        f"{what}: {float(np.abs(a - b).max()):.3e} of {float(np.abs(b).max()):.3e}"


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}d-{c[2]}-q{'x'.join(map(str, c[3]))}k{'x'.join(map(str, c[4]))}")
def test_one_part_is_the_oracle(case, dtype):
    policy, seq, mode, qs, ks, ws, ls, causal = case
    prob = O.Problem(policy, seq, mode, ws, ls, causal)
    b, d, vd, nq, nk = 2, 24, 40, int(np.prod(qs)), int(np.prod(ks))
    Q, (K,), (V,), dO = _inputs(dtype, b, d, vd, nq, [nk], seed=nq + nk)
    shaped = lambda x, s: x.reshape(x.shape[:2] + s)  # noqa: E731
    args = (shaped(Q, qs), shaped(K, ks), shaped(V, ks))
    u_t, u_acc = U_ROUND[dtype]
    mask = O.problem_mask(prob, qs, ks)
    r = union_ref.union(Q, [K], [V], dO, [mask], u_t, u_acc)
    o, L, M, ha = O.forward_f64(*args, prob)
    assert np.array_equal(r["ha"], ha)
    _same(r["O"], o.reshape(b, vd, nq), "O"); _same(r["L"], L.reshape(b, nq), "L"); _same(r["M"], M.reshape(b, nq), "M")
    for name, x, y in zip(("dQ", "dK", "dV"), (r["dQ"], r["dKs"][0], r["dVs"][0]), O.backward_f64(*args, shaped(dO, qs), prob)):
        _same(x, y.reshape(x.shape), name)
    for name, x, y in zip(("eQ", "eK", "eV"), (r["eQ"], r["eKs"][0], r["eVs"][0]),
                          O.backward_rounding_scale_f64(*args, shaped(dO, qs), prob, u_t, u_acc)):
        _same(x, y.reshape(x.shape), name)
    _same(r["dQ_parts"][0], r["dQ"], "the only part's dQ")
    # what a forward stores: the oracle's own (O, l, m), rows without a key included
    for x, y in zip(union_ref.stored(r, dtype), O.forward(*args, prob)):
        assert x.dtype == y.dtype
        if (~ha).any():
            assert x[..., ~ha].tobytes() == y.reshape(x.shape)[..., ~ha].tobytes()
        _same(x[..., ha], y.reshape(x.shape)[..., ha], "stored")
    if (~ha).any():
        m = union_ref.stored(r, dtype)[2]
        assert m[:, ~ha].tobytes() == b"\xfa" * (m[:, ~ha].size * np.dtype(dtype).itemsize)
        assert (r["dQ"][:, :, ~ha] == 0).all() and (r["eQ"][:, :, ~ha] == 0).all()


def test_some_cases_have_rows_without_a_key():
    n = 0
    for policy, seq, mode, qs, ks, ws, ls, causal in CASES:
        ha = O.problem_mask(O.Problem(policy, seq, mode, ws, ls, causal), qs, ks).any(axis=1)
        n += bool(0 < (~ha).sum() < ha.size)
    assert n >= 3


def test_two_parts_are_the_inline_reference_of_the_merge_tests():
    from tests import test_gpu_merge as gm
    name = "window_global_f32"
    dtype, seq, qs, d, vd, specs = gm.CASES[name]
    c = gm.case_data(name)
    b, nq = c["b"], c["nq"]
    flat = lambda x: x.reshape(b, x.shape[len(gm.BATCH)], -1)  # noqa: E731
    r = union_ref.union(flat(c["Q"]), [flat(x) for x in c["Ks"]], [flat(x) for x in c["Vs"]], flat(c["dO"]), c["masks"],
                        *U_ROUND[dtype])
    assert np.array_equal(r["mask"], c["mask"]) and np.array_equal(r["ha"], c["ha"])
    for key in ("O", "L", "M", "dQ"):
        _same(r[key], c[key], key)
    for j in range(len(specs)):
        _same(r["dKs"][j], c["dKs"][j], f"dK{j}"); _same(r["dVs"][j], c["dVs"][j], f"dV{j}")
        _same(np.abs(r["dQ_parts"][j]).max(), c["dq_part_max"][j], f"max |dQ_{j}|")
    _same(r["dQ_parts"].sum(axis=0), r["dQ"], "the sum of the parts' dQ")
    # a part alone: the statistics mutation (a) of tests/test_union_fuzz_draws.py starts from
    for j, s in enumerate(specs):
        o, L, M, ha = union_ref.part_statistics(flat(c["Q"]), flat(c["Ks"][j]), flat(c["Vs"][j]), c["masks"][j])
        ref = O.forward_f64(c["Q"].reshape((b, d) + qs), c["Ks"][j].reshape((b, d) + s.ks), c["Vs"][j].reshape((b, vd) + s.ks),
                            s.problem(seq))
        _same(o, ref[0].reshape(o.shape), "O_i"); _same(L, ref[1].reshape(L.shape), "L_i"); _same(M, ref[2].reshape(M.shape), "M_i")


@pytest.mark.parametrize("g,bkv", [(2, 3), (8, 1)])
def test_grouped_helper_is_the_fold_of_the_expanded_problem(g, bkv):
    """tests/test_gpu_grouped.py::test_gradients' reference: np.repeat, the oracle, dK / dV summed over each group in
    float64, the root-sum-square of the members' scales."""
    dtype, d, vd, nq, nk = np.float16, 32, 24, 9, 70
    rng = np.random.default_rng(g)
    u = lambda *s: rng.uniform(-2, 2, s).astype(dtype)  # noqa: E731
    Q, dO, K, V = u(bkv * g, d, nq), u(bkv * g, vd, nq), u(bkv, d, nk), u(bkv, vd, nk)
    prob = O.Problem("local", 1, "scale_front", 20, 0, True)
    u_t, u_acc = U_ROUND[dtype]
    r = union_ref.grouped(Q, K, V, dO, O.problem_mask(prob, (nq,), (nk,)), g, u_t, u_acc)
    Ke, Ve = np.repeat(K, g, axis=0), np.repeat(V, g, axis=0)
    dQ, dKe, dVe = O.backward_f64(Q, Ke, Ve, dO, prob)
    eQ, eKe, eVe = O.backward_rounding_scale_f64(Q, Ke, Ve, dO, prob, u_t, u_acc)
    fold = lambda x: x.reshape((bkv, g) + x.shape[1:]).sum(axis=1)  # noqa: E731
    rss = lambda e: np.sqrt((e.reshape((bkv, g) + e.shape[1:]) ** 2).sum(axis=1))  # noqa: E731
    for name, x, y in (("O", r["O"], O.forward_f64(Q, Ke, Ve, prob)[0]), ("dQ", r["dQ"], dQ), ("eQ", r["eQ"], eQ),
                       ("dK", r["dK"], fold(dKe)), ("dV", r["dV"], fold(dVe)), ("eK", r["eK"], rss(eKe)), ("eV", r["eV"], rss(eVe))):
        _same(x, y, name)
    assert r["dK"].shape == K.shape and r["dV"].shape == V.shape
    _same(r["dKe"].sum(axis=1), r["dK"], "members")


def test_the_underflow_step_only_adds():
    """eta (half a subnormal step of T; tests/test_gpu_union_fuzz.py) enlarges every scale of an allowed pair and
    leaves the reference itself alone; eta = 0 is the oracle's formula."""
    Q, Ks, Vs, dO = _inputs(np.float16, 1, 8, 8, 12, [12, 5], seed=4)
    masks = [O.problem_mask(O.Problem("causal", 1, "none_front"), (12,), (12,)), np.ones((12, 5), bool)]
    u_t, u_acc = U_ROUND[np.float16]
    a = union_ref.union(Q, Ks, Vs, dO, masks, u_t, u_acc)
    b = union_ref.union(Q, Ks, Vs, dO, masks, u_t, u_acc, eta=2.0 ** -25)
    for key in ("O", "L", "M", "dQ"):
        assert np.array_equal(a[key], b[key])
    for key in ("eKs", "eVs"):
        assert all((y > x).all() for x, y in zip(a[key], b[key]))
    assert (b["eQ"] > a["eQ"]).all() and (b["eQ"] < a["eQ"] + 1e-5).all()
