"""Dense float64 reference of one Q attending a concatenated key set under an arbitrary boolean mask: what
combined_1d / combined_2d compute over the union of their parts and, on K / V repeated per
group, what grouped_1d / grouped_2d compute (§3.8).  Test infrastructure only; nothing here comes from the code
under test.

union(Q, Ks, Vs, dO, masks, u_t, u_acc): Q [b, d, nq], part i's K_i [b, d, nk_i], V_i [b, v_d, nk_i] and mask
[nq, nk_i], dO [b, v_d, nq], all already flattened.  One softmax at scale 1/sqrt(d) over every allowed key of every
part; the gradients taken analytically (D = rowsum(dO*O), dS = P*(dP - D)*scale, as oracle.backward_f64); the
per-part dQ_i = K_i dS_i^T whose sum is dQ; and the per-element rounding scales of
oracle.backward_rounding_scale_f64, the same formula term for term with P, O and D of the union.  A row that no
part allows a key has O = 0, L = 0, M = 0 and no gradient; stored(ref, dtype) gives the (O, l, m) a forward stores
for the reference, such rows as O = 0, l = 0, m = bytes 0xFA.

Two optional terms extend the oracle's rounding model for the sweep's offset inputs (tests/test_gpu_union_fuzz.py);
both are 0 by default, and the scales are then the oracle's to the last bits (tests/test_union_ref.py):
  eta    half a subnormal step of T.  A value stored in T below T's normal range is rounded by up to eta absolutely,
         not by u_t relatively: the P and dS of a part whose scores lie 12 below the row's max (exp(-12) = 6e-6, in
         fp16's subnormal range) and its stored gradients.  Every allowed pair's P and dS and every stored gradient
         get eta beside their relative term.  Without it a dK of 1e-9 that fp16 stores as 0 fails the slope check
         (slope -1: the float64 reference itself, rounded to fp16, in 11 of the 120 default fp16 cases, first seed 12, dK of
         a part 12 below the max).
  carry  [b, nk]: the part of a score, |q_0 k_0| / sqrt(d), that the accumulator carries through the fma chain of
         its d products because it enters first.  The oracle's u_t * |s|_rss rounds every product once; a chain
         that holds a partial sum of size c rounds it d times, u_acc * c each: u_acc * sqrt(d) * c in all, which
         the score's (and P's relative) scale gets.  With U(-2, 2) inputs the partial sums are of the size of
         |s|_rss and the term is in the oracle's; with K's channel 0 at delta * sqrt(d) / 2 it is |delta| for all
         d steps.  Measured over the default range before the term (fp32, 20 of 60 cases past the bound, every one
         in dQ's channel 0 = k_0 * sum_k dS_k, which is 0 analytically in a grouped case): worst error / bound
         3.02 at seed 186 (d = 288, offsets +-12); the relative error of P that those errors imply, 1.0e-6
         (d = 32, offset 12; seed 67), 2.0e-6 (d = 100, 12; seed 235), 2.8e-6 (d = 288, 12; seed 219) in the median
         row, follows sqrt(d) * |delta| at a third of this bound.  A float32 numpy evaluation, whose blocked sums
         do not carry the offset, stays 10 x lower in that channel and equal in every other.

grouped(Q, K, V, dO, mask, g, u_t, u_acc): Q [bkv * g, d, nq] against K [bkv, d, nk], V [bkv, v_d, nk]; query slice
h reads K/V slice h // g (np.repeat), dK / dV are folded over each group in float64 and their scales are the
root-sum-square of the members' scales."""
import math

import numpy as np

from oracle import fa_oracle as O


def union(Q, Ks, Vs, dO, masks, u_t, u_acc, eta=0.0, carry=None):
    """dict: O [b, v_d, nq], L, M [b, nq], ha [nq] (rows with a key), dQ [b, d, nq], dQ_parts [n, b, d, nq], eQ, and
    per part the lists dKs, dVs, eKs, eVs; mask [nq, nk_total] and edges (the parts' column ranges)."""
    Q = np.asarray(Q, dtype=np.float64)
    dO = np.asarray(dO, dtype=np.float64)
    b, d, nq = Q.shape
    n = len(Ks)
    nks = [int(x.shape[2]) for x in Ks]
    edges = np.cumsum([0] + nks)
    mask = np.concatenate([np.asarray(mk, dtype=bool).reshape(nq, nk) for mk, nk in zip(masks, nks)], axis=1)
    k = np.concatenate([np.asarray(x, dtype=np.float64) for x in Ks], axis=2)
    v = np.concatenate([np.asarray(x, dtype=np.float64) for x in Vs], axis=2)
    vd = v.shape[1]
    scale = 1.0 / math.sqrt(d)
    ha = mask.any(axis=1)
    o = np.zeros((b, vd, nq)); L = np.zeros((b, nq)); M = np.zeros((b, nq))
    dq = np.zeros((b, d, nq)); dk = np.zeros_like(k); dv = np.zeros_like(v)
    eq = np.zeros((b, d, nq)); ek = np.zeros_like(k); ev = np.zeros_like(v)
    dq_parts = np.zeros((n, b, d, nq))
    for i in range(b):
        qi, ki, vi, doi = Q[i], k[i], v[i], dO[i]
        s = np.where(mask, (qi.T @ ki) * scale, -np.inf)
        mrow = np.where(ha, s.max(axis=1, initial=-np.inf), 0.0)
        p = np.exp(s - mrow[:, None])
        lrow = p.sum(axis=1)
        p = p / np.where(ha, lrow, 1.0)[:, None]            # 0 where masked
        o[i] = vi @ p.T
        L[i], M[i] = np.where(ha, lrow, 0.0), mrow
        dv[i] = doi @ p
        dp = doi.T @ vi
        D = np.sum(doi * o[i], axis=0)
        ds = p * (dp - D[:, None]) * scale
        dq[i] = ki @ ds.T
        dk[i] = qi @ ds
        for j in range(n):
            c0, c1 = edges[j], edges[j + 1]
            dq_parts[j, i] = ki[:, c0:c1] @ ds[:, c0:c1].T
        # oracle.backward_rounding_scale_f64, term for term
        s_rss = np.sqrt((qi * qi).T @ (ki * ki)) * scale
        e_p = (u_t * (1.0 + s_rss) + (0.0 if carry is None else u_acc * math.sqrt(d) * carry[i][None, :])) * p + eta * mask
        e_ds = scale * (e_p * np.abs(dp - D[:, None])
                        + p * (u_t * np.sqrt(np.sum((doi * o[i]) ** 2, axis=0))[:, None]
                               + u_acc * (np.abs(doi).T @ np.abs(vi)))) + eta * mask
        ev[i] = (doi * doi) @ (e_p * e_p)
        eq[i] = (ki * ki) @ (e_ds * e_ds).T
        ek[i] = (qi * qi) @ (e_ds * e_ds)
    eq, ek, ev = np.sqrt(eq + eta * eta), np.sqrt(ek + eta * eta), np.sqrt(ev + eta * eta)
    cut = lambda x: [x[:, :, edges[j]:edges[j + 1]] for j in range(n)]  # noqa: E731
    return dict(O=o, L=L, M=M, ha=ha, dQ=dq, dKs=cut(dk), dVs=cut(dv), dQ_parts=dq_parts, eQ=eq, eKs=cut(ek),
                eVs=cut(ev), mask=mask, edges=edges)


def part_statistics(Q, K, V, mask):
    """(O_i, L_i, M_i, ha_i) of one part alone: the forward of that part's own problem, in float64."""
    r = union(Q, [K], [V], np.zeros((Q.shape[0], V.shape[1], Q.shape[2])), [mask], 0.0, 0.0)
    return r["O"], r["L"], r["M"], r["ha"]


def stored(ref, dtype):
    """(O, l, m) as a forward stores the reference's values: O in T, m the row max rounded to T, l in L_T relative
    to the stored m; the rows without a key O = 0, l = 0, m = NegInfApprox."""
    ha = ref["ha"]
    m_t = ref["M"].astype(dtype)
    l = np.where(ha[None, :], ref["L"] * np.exp(ref["M"] - m_t.astype(np.float64)), 0.0).astype(O.l_dtype_for(dtype))
    m = np.where(ha[None, :], m_t, O.neg_inf_approx(dtype)).astype(dtype)
    return ref["O"].astype(dtype), l, m


def grouped(Q, K, V, dO, mask, g, u_t, u_acc, eta=0.0, carry=None):
    """The reference of a grouped call: union() of one part on K / V repeated g times along the slices; dK / dV
    folded over each group in float64, eK / eV the root-sum-square of the members' scales.  dict: O, L, M, ha, dQ,
    eQ, dK, dV, eK, eV (K's and V's own shapes) and the unfolded dKe, dVe [bkv, g, ., nk]."""
    bkv = K.shape[0]
    r = union(Q, [np.repeat(K, g, axis=0)], [np.repeat(V, g, axis=0)], dO, [mask], u_t, u_acc, eta,
              None if carry is None else np.repeat(carry, g, axis=0))
    members = lambda x: x.reshape((bkv, g) + x.shape[1:])  # noqa: E731
    fold = lambda x: members(x).sum(axis=1)  # noqa: E731
    rss = lambda e: np.sqrt((members(e) ** 2).sum(axis=1))  # noqa: E731
    return dict(O=r["O"], L=r["L"], M=r["M"], ha=r["ha"], dQ=r["dQ"], eQ=r["eQ"], dK=fold(r["dKs"][0]),
                dV=fold(r["dVs"][0]), eK=rss(r["eKs"][0]), eV=rss(r["eVs"][0]), dKe=members(r["dKs"][0]),
                dVe=members(r["dVs"][0]), mask=r["mask"])
