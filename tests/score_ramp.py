"""Staircase-score inputs for the forwards' lazy softmax rebase (plain numpy, no GPU).

Every forward kernel keeps its online-softmax reference m_run lazily: it moves only when a tile's row
max passes it by more than a threshold (8 log2 units in the fp16 / fp32 kernels, 16 natural units in
fa_f64.hip).  U(-2, 2) inputs never take that branch after the seed.  These inputs make the scores of
every row a staircase along the key axis, so the branch runs on chosen tiles, while the documented fp16
deviation (scores formed from Q·scale·log2e rounded to fp16) stays as small as on the
usual inputs.

Construction.  Keys are cut into plateaus of W consecutive flat indices, t(k) = k // W, T plateaus in
all; plateau t has the exponent e(k) = min(T-1-t, E).  Two channels are special:

    K[0, k] = -u·2^e(k)        K[1, k] = 1
    climb rows:  Q[0, q] = q0,  Q[1, q] = q0·u·2^e(kmax(q))       kmax = the row's highest allowed key

and the fall rows use the mirror image in two channels of their own, f(k) = min(t(k), F):

    K[3, k] = -u·2^f(k)        K[4, k] = 1
    fall rows:   Q[3, q] = q0,  Q[4, q] = q0·u·2^f(kmin(q))       kmin = the row's lowest allowed key

(each row kind has zeros in the other kind's pair, flat rows in both).  The pair adds
-q0·u·(2^e(k) - 2^e(top)) / sqrt(d) to a score: 0 on the row's top plateau, and steps of σ0·2^j log2 units
(σ0 = q0·u·scale·log2e) below it.  A climb row's scores rise with the key index up to its last allowed
key, whatever the rule; a fall row's top is its first plateau and the later tiles sink by σ0, 3σ0, 7σ0
and 15σ0 (F = 4: P is 0 in fp16 and below 1e-12 elsewhere; a larger F would only put large K beside the
climb rows' tops, where their zero-valued Q[3] turns dQ[3] into a sum of cancelling K·dS terms that
fp32 cannot hold to the backward gate); a flat row never leaves its seed.

u is a power of two, so every special value is a power of two times q0 (or, after the kernels'
pre-scaling of Q by c = scale·log2e, or of K in the fp16 dK / dV pass, times fl(q0·c) or fl(c)):
rounding commutes with it, and the two products of a top-plateau score cancel exactly in the
kernel's own arithmetic.  The accumulator holds them for a moment, though:
the score is then rounded at their magnitude, σ0·2^e(top) log2 units.  Under the full policy e(top) = 0
for every row; under the other rules it reaches E, which costs 2^-24·σ0·2^E ≈ 1e-4 in fp32, so the
fp32 cases use the full policy (fp16's own rounding and fp64's are far from it).

The other channels of K are U(-a, a) noise with a <= 0.25 (so a plateau is not bitwise flat); Q
elsewhere, V and dO are U(-2, 2) as in every other test.  The three row kinds are
interleaved (q % 4), so the kernels' wave-uniform `__any` branch runs with lanes that must not move.

A third channel lifts every score of every row by the same amount, about `lift` log2 units: K[2, k] = κ,
Q[2, q] = L.  The kernels start m_run at 0, so a staircase whose top sits at 0 is computed correctly even
by a kernel that never seeds or rebases; with the lift the seed and the rebases carry the result (a P
of 2^24 overflows fp16).  A uniform shift cancels in O and in l (stored relative to the stored m) only if
the kernel's shift equals the exact one, so κ in [1, 2) and L near lift / (κ·scale·log2e) are the fp16
values whose pre-scaled fp16 images are closest to exact (lift_pair: relative residuals of ~1e-6
instead of 2^-12; the forward and the dQ pass pre-scale Q, the dK / dV pass pre-scales K).

Also here: a numpy model of the lazy rebase (which tiles of which rows take the branch), an emulation of
the documented fp16 deviation with the checks run_case applies, and the table of cases that
tests/test_gpu_score_range.py runs and tests/test_score_ramp_inputs.py vets on the CPU; and, at the end, the
same for the few-query decode forwards (DECODE_CASES: tests/test_gpu_decode_score_range.py,
tests/test_decode_score_ramp_inputs.py).
"""

import math
from dataclasses import dataclass, field

import numpy as np

from oracle import fa_oracle as O
from tests import gate

LOG2E = 1.4426950408889634
CLIMB, FLAT, FALL = 0, 1, 2
N_SPECIAL = 5                             # channels 0-4 are constructed, the rest are noise
KIND_CYCLE = (CLIMB, FLAT, CLIMB, FALL)   # row q is of kind KIND_CYCLE[q % 4]


@dataclass
class Ramp:
    """W keys a plateau; the special channels' q0, u (a power of two) and exponent caps E (climb) and F
    (fall); noise width a; lift in log2 units."""
    W: int
    q0: float = 2.0
    u: float = 8.0
    E: int = 10
    F: int = 4
    a: float = 0.25
    lift: float = 24.0

    def sigma0(self, d):
        """The smallest step, in log2 units."""
        return self.q0 * self.u * LOG2E / math.sqrt(d)


def _best_prescaled(d, lo, hi):
    """The fp16 value x in [lo, hi] whose image under the fp16 kernels' pre-scaling,
    fp16(f32(x)·f32(f32(scale)·f32(log2e))), has the smallest relative distance from x·scale·log2e."""
    c = LOG2E / math.sqrt(d)
    c2 = np.float32(np.float32(1.0 / math.sqrt(d)) * np.float32(LOG2E))
    lo, hi = np.float16(lo), np.float16(hi)
    cand = np.arange(lo.view(np.uint16), hi.view(np.uint16) + 1, dtype=np.uint16).view(np.float16)
    img = (cand.astype(np.float32) * c2).astype(np.float16).astype(np.float64)
    exact = cand.astype(np.float64) * c
    return float(cand[np.argmin(np.abs(img - exact) / exact)])


def lift_pair(d, lift):
    """(L, κ) of the lift channel: Q[2] = L, K[2] = κ, L·κ·scale·log2e within 1/8 of `lift`."""
    if not lift:
        return 0.0, 0.0
    kappa = _best_prescaled(d, 1.0, 1.999)
    target = lift * math.sqrt(d) / LOG2E / kappa
    return _best_prescaled(d, target * 0.875, target * 1.125), kappa


def plateau_exponents(nk, ramp, mirror=False):
    t = np.arange(nk) // ramp.W
    return np.minimum(t, ramp.F) if mirror else np.minimum(t.max() - t, ramp.E)


def row_tops(mask):
    """(kmax, kmin, has_any) per query row of a bool [nq, nk] mask; rows without a key get 0."""
    has = mask.any(axis=1)
    kmin = np.where(has, mask.argmax(axis=1), 0)
    kmax = np.where(has, mask.shape[1] - 1 - mask[:, ::-1].argmax(axis=1), 0)
    return kmax, kmin, has


def ramp_inputs(prob, dtype, batch, d, vd, qs, ks, ramp, seed=0, mask=None, row0=0):
    """(Q, K, V, dO) of the given dtype and a dict with the row kinds, each row's top key and the mask.
    mask (optional, bool [nq, nk]) stands in for the one derived from prob; row0 shifts the cycle of the row
    kinds (row q is of kind KIND_CYCLE[(row0 + q) % 4]: the decode cases cycle over the folded row index)."""
    assert d >= 6 and float(ramp.u) == 2.0 ** round(math.log2(ramp.u))
    rng = np.random.default_rng(seed)
    batch, qs, ks = tuple(batch), tuple(qs), tuple(ks)
    nq, nk = int(np.prod(qs)), int(np.prod(ks))
    b = int(np.prod(batch))
    Q = rng.uniform(-2, 2, (b, d, nq))
    K = rng.uniform(-ramp.a, ramp.a, (b, d, nk))
    V = rng.uniform(-2, 2, (b, vd, nk))
    dO = rng.uniform(-2, 2, (b, vd, nq))
    mask = O.problem_mask(prob, qs, ks) if mask is None else np.asarray(mask, dtype=bool)
    kmax, kmin, has = row_tops(mask)
    e, f = plateau_exponents(nk, ramp), plateau_exponents(nk, ramp, mirror=True)
    kind = np.array(KIND_CYCLE)[(row0 + np.arange(nq)) % 4]
    kind = np.where(has, kind, FLAT)            # rows that attend nothing keep their sentinels
    top = np.where(kind == FALL, kmin, kmax)
    K[:, 0, :], K[:, 3, :] = -ramp.u * 2.0 ** e, -ramp.u * 2.0 ** f
    K[:, 1, :] = K[:, 4, :] = 1.0
    Q[:, 0, :] = np.where(kind == CLIMB, ramp.q0, 0.0)
    Q[:, 1, :] = np.where(kind == CLIMB, ramp.q0 * ramp.u * 2.0 ** e[top], 0.0)
    Q[:, 3, :] = np.where(kind == FALL, ramp.q0, 0.0)
    Q[:, 4, :] = np.where(kind == FALL, ramp.q0 * ramp.u * 2.0 ** f[top], 0.0)
    Q[:, 2, :], K[:, 2, :] = lift_pair(d, ramp.lift)
    tope = np.where(kind == FALL, f[top], e[top])
    on_top = np.where((kind == FALL)[:, None], f[None, :] == tope[:, None], e[None, :] == tope[:, None]) & mask
    out = tuple(x.reshape(batch + x.shape[1:2] + s).astype(dtype) for x, s in ((Q, qs), (K, ks), (V, ks), (dO, qs)))
    return out, dict(kind=kind, top=top, mask=mask, has=has, on_top=on_top)


def _flat3(x, seq_dims):
    lead = x.ndim - seq_dims - 1
    return x.reshape((int(np.prod(x.shape[:lead])) if lead else 1, x.shape[lead], -1))


# ---------------------------------------------------------------------------------- the rebase model
def rebase_tiles(scores, mask, tile, thr):
    """Which tiles of which rows take the lazy-rebase branch after the seed.

    scores [nq, nk] in the kernel's units, mask [nq, nk]; tiles are `tile` keys wide and start at key 0,
    as in every kernel's key loop.  The model is the kernels' rule for one row: the first tile with an
    allowed key seeds m_run with its row max; a later tile whose row max exceeds m_run by more than thr
    moves m_run to that max.  (A kernel also moves the other lanes of a wave that takes the branch, by
    their own max(mt, 0); that is what the interleaved flat and fall rows check, not this count.)
    Returns (rebased [nq, ntiles] bool, active [nq, ntiles] bool: the tile holds an allowed key)."""
    nq, nk = scores.shape
    nt = (nk + tile - 1) // tile
    s = np.where(mask, scores, -np.inf)
    pad = nt * tile - nk
    if pad:
        s = np.concatenate([s, np.full((nq, pad), -np.inf)], axis=1)
    tmax = s.reshape(nq, nt, tile).max(axis=2)
    active = np.isfinite(tmax)
    rebased = np.zeros((nq, nt), dtype=bool)
    m_run = np.full(nq, np.nan)
    for t in range(nt):
        seed = np.isnan(m_run) & active[:, t]
        with np.errstate(invalid="ignore"):
            move = ~np.isnan(m_run) & active[:, t] & (tmax[:, t] - m_run > thr)
        rebased[:, t] = move
        m_run = np.where(seed | move, tmax[:, t], m_run)
    return rebased, active


def rebase_conditions(rebased, active, kind):
    """The conditions a case must meet (tests/test_score_ramp_inputs.py), as a dict of booleans.

    Among the climb rows: a rebase on two consecutive active tiles of one row; a rebase on a row's last
    active tile; a stretch of at least two active tiles after the seed without one.  No flat or fall row
    rebases at all."""
    consecutive = last = quiet = False
    for q in np.nonzero(kind == CLIMB)[0]:
        act = np.nonzero(active[q])[0]
        if act.size < 2:
            continue
        r = rebased[q, act[1:]]                     # the active tiles after the seed
        consecutive |= bool((r[1:] & r[:-1]).any())
        last |= bool(r[-1])
        quiet |= bool((~r[1:] & ~r[:-1]).any())
    return dict(consecutive=consecutive, last=last, quiet=quiet,
                others_still=not rebased[kind != CLIMB].any(),
                n=int(rebased[kind == CLIMB].sum()))


def kernel_scores(Q, K, d, log2_units):
    """float64 scores [nq, nk] of slice 0 in the kernel's units (log2 for fp16 / fp32, natural for fp64)."""
    q, k = Q[0].astype(np.float64), K[0].astype(np.float64)
    return (q.T @ k) * ((LOG2E if log2_units else 1.0) / math.sqrt(d))


# ------------------------------------------------------------------- the tight bound on m's rounding
def m_rounding_bound(Q, K, info, dtype, d):
    """[b, nq]: how far rounding can move a row's max on these inputs; run_case takes it in place of its
    dot-product term, which |Q[1]| up to 16384 would make vacuous.

    A row's max sits on its top plateau (the next one is at least σ0 >= 2 log2 units lower, the noise
    spans a fraction of that).  fp32 / fp64: sqrt(d) units of the type's rounding of scale·Σ_c|q_c·k_c| over
    the top plateau's keys only, special channels included (their products cancel exactly, but the
    accumulator holds them while the noise terms are added).  run_case takes 2 units of a sum that is far
    above the score; here the lift keeps the partial sum at the score's size through all d
    additions, each rounding it by up to eps/2, so the random-walk bound sqrt(d)·eps/2 with a factor of
    two stands in (at a lift of 24 the 300-channel SIMT fp32 forward reached 14 eps of m).  fp16: the pre-scaled Q's
    2^-11 and the f32 accumulation's d·2^-24 on the noise channels' Σ_c|q_c·k_c|, plus the packed-P max
    approximation 4.9e-4: the two special products are exact in f32 (11-bit factors times
    powers of two), neighbours in the first MFMA of the chain, and cancel there; the lift channel's
    pre-scaled value is exact to ~1e-6 by construction (lift_pair), far inside the 1e-3·|m| floor."""
    b, _, nq = Q.shape
    on_top, has = info["on_top"], info["has"]
    out = np.zeros((b, nq))
    scale = 1.0 / math.sqrt(d)
    c0 = N_SPECIAL if dtype == np.float16 else 0
    for i in range(b):
        aq = np.abs(Q[i, c0:].astype(np.float64)).T
        ak = np.abs(K[i, c0:].astype(np.float64))
        out[i] = np.where(on_top, aq @ ak, 0.0).max(axis=1) * scale
    if dtype == np.float16:
        return np.where(has, (2.0 ** -11 + d * 2.0 ** -24) * out + 4.9e-4, 0.0)
    return max(2.0, math.sqrt(d)) * float(np.finfo(dtype).eps) * out


# ------------------------------------------------------------- the documented fp16 deviation, emulated
def emulate_f16(Q, K, V, dO, prob, qs, ks, bwd):
    """What a correct fp16 kernel computes, in float64 except for its documented roundings: Q pre-scaled
    by float(scale)·log2e in f32 and rounded to fp16, P rounded to fp16 (row sums taken over the rounded
    values), O and m rounded to fp16, l relative to the stored m in f32; backward: P recomputed from the
    stored m and l, with the scores of the dQ pass from the pre-scaled Q and those of the dK / dV pass
    from K pre-scaled the same way (fa_bwd_f16_fast.hip), P and dS rounded to fp16, gradients rounded
    to fp16.  Inputs [b, ch, n]."""
    b, d, nq = Q.shape
    mask = O.problem_mask(prob, qs, ks)
    has = mask.any(axis=1)
    scale = 1.0 / math.sqrt(d)
    c2 = np.float32(np.float32(scale) * np.float32(LOG2E))
    out = dict(O=[], l=[], m=[], dQ=[], dK=[], dV=[])
    for i in range(b):
        qs16 = (Q[i].astype(np.float32) * c2).astype(np.float16).astype(np.float64)
        k, v = K[i].astype(np.float64), V[i].astype(np.float64)
        s2 = np.where(mask, qs16.T @ k, -np.inf)
        m2 = np.where(has, s2.max(axis=1), 0.0)
        p16 = np.exp2(s2 - m2[:, None]).astype(np.float16).astype(np.float64)
        l_run = np.where(has, p16.sum(axis=1), 1.0)
        o16 = ((v @ p16.T) / l_run).astype(np.float16)
        m16 = (m2 / LOG2E).astype(np.float16)
        l32 = (l_run * np.exp2(m2 - m16.astype(np.float64) * LOG2E)).astype(np.float32)
        out["O"].append(np.where(has, o16, 0)); out["l"].append(np.where(has, l32, 0)); out["m"].append(m16)
        if not bwd:
            continue
        do = dO[i].astype(np.float64)
        q = Q[i].astype(np.float64)
        lse = m16.astype(np.float64) * LOG2E + np.log2(np.where(has, l32.astype(np.float64), 1.0))
        dpd = (do.T @ v - np.sum(do * o16.astype(np.float64), axis=0)[:, None]) * scale
        # dQ pass: scores from the pre-scaled Q, as in the forward
        pq = np.exp2(s2 - lse[:, None])
        out["dQ"].append((k @ (pq * dpd).astype(np.float16).astype(np.float64).T).astype(np.float16))
        # dK / dV pass: scores from K pre-scaled the same way
        ks16 = (K[i].astype(np.float32) * c2).astype(np.float16).astype(np.float64)
        pk = np.exp2(np.where(mask, q.T @ ks16, -np.inf) - lse[:, None])
        out["dV"].append((do @ pk.astype(np.float16).astype(np.float64)).astype(np.float16))
        out["dK"].append((q @ (pk * dpd).astype(np.float16).astype(np.float64)).astype(np.float16))
    return {n: np.stack(x) for n, x in out.items() if x}, has


def gate_ratios(case, inputs, info, got, has):
    """Worst |error| / allowance of the emulated outputs under run_case's checks of O, l and m (m with
    the tight bound), and, if `got` holds gradients, under gate.grad_bound and the slope check."""
    dtype, prob, sd = case.dtype, case.problem(), case.seq_dims
    Qb, Kb, Vb, dOb = (x.reshape((-1,) + x.shape[x.ndim - sd - 1:]) for x in inputs)   # [b, ch, *seq]
    Q, K = _flat3(Qb, sd), _flat3(Kb, sd)
    O64, L64, M64, _ = O.forward_f64(Qb, Kb, Vb, prob)
    b, nq = Q.shape[0], Q.shape[2]
    O64, L64, M64 = O64.reshape(b, -1, nq), L64.reshape(b, nq), M64.reshape(b, nq)
    rtol, atol = gate.TOL[dtype]["fwd"]
    res = {"O": float((np.abs(got["O"].astype(np.float64) - O64) / gate.plain_bound(O64, rtol, atol)).max())}
    m_f = got["m"].astype(np.float64)[:, has]
    tol = gate.m_tol_bounded(M64[:, has], dtype, m_rounding_bound(Q, K, info, dtype, case.d)[:, has])
    res["m"] = float((np.abs(m_f - M64[:, has]) / tol).max())
    l_ref = L64[:, has] * np.exp(M64[:, has] - m_f)
    res["l"] = float((np.abs(got["l"].astype(np.float64)[:, has] - l_ref) / gate.plain_bound(l_ref, rtol, atol)).max())
    if "dQ" in got:
        refs = O.backward_f64(Qb, Kb, Vb, dOb, prob)
        es = O.backward_rounding_scale_f64(Qb, Kb, Vb, dOb, prob, *gate.U_ROUND[dtype])
        for name, ref, e in zip(("dQ", "dK", "dV"), refs, es):
            ref, e = _flat3(ref, sd), _flat3(e, sd)
            g = got[name].astype(np.float64)
            res[name] = float((np.abs(g - ref) / gate.grad_bound(ref, e, dtype)).max())
            if gate.slope_applies(ref, e):
                res[name + "_slope"] = abs(gate.scale_slope(g, ref)) / gate.slope_tol_eff(ref, e, dtype, case.d, g.shape[1])
    return res


# ------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    """One GPU case: the problem, the ramp, the kernel's tile width and threshold (for the rebase
    model), whether the backward is checked, and how the forward is routed."""
    id: str
    dtype: type
    policy: str
    mode: str
    d: int
    vd: int
    qs: tuple
    ks: tuple
    ramp: Ramp
    tile: int
    ws: int = 1
    ls: int = 0
    causal: bool = False
    bwd: bool = True
    variant: str = ""          # FA_FWD_VARIANT of the diagnostic library ("" = the product library)
    split: bool = False        # the split-key forward: fa_forward_split_plan must report >= 2 chunks
    batch: tuple = (2,)
    seed: int = 0
    waive: tuple = field(default_factory=tuple)   # conditions the shape cannot meet (reason beside the case)

    @property
    def seq_dims(self):
        return len(self.qs)

    @property
    def log2_units(self):
        return self.dtype != np.float64

    @property
    def thr(self):
        return 8.0 if self.log2_units else 16.0

    def problem(self):
        return O.Problem(self.policy, self.seq_dims, self.mode, self.ws, self.ls, self.causal)

    def inputs(self):
        return ramp_inputs(self.problem(), self.dtype, self.batch, self.d, self.vd, self.qs, self.ks, self.ramp,
                           self.seed)


# The ramps.  A climb row of the full policy steps up by ..., 8σ0, 4σ0, 2σ0, σ0 towards its top.  With
# 8/3 < σ0 <= 4 (in the kernel's units, threshold 8; fp64: 16/3 < σ0 <= 8 natural units, threshold 16)
# the 4σ0 step and every larger one rebase, the 2σ0 step does not, and σ0 on the last tile does,
# because 3σ0 has then accumulated: two consecutive rebases, a quiet tile and a rebase on the ragged
# last tile in one row.  The plateaus more than E below the top share one level (the quiet stretch), and
# the steps next to it are σ0·2^(E-1) > 128: the fp32 exp2 of a speculative exponential overflows there.
# q0, u and E per channel count keep max|Q| = q0·u·2^E and max|K| = u·2^E at or below 16384.
def _ramp(d, W, dtype, big=False, E=None):
    """big: the second, doubled σ0 (the last tile's step alone then stays under the threshold for a
    full-policy row, so it is used where the rows' tops differ: causal and windowed rules).  The lift is
    24 log2 units in fp16 (past fp16's largest P, 2^16) and 4 in fp32 / fp64: there it only has to move the
    top off m_run's initial 0, and a d-term dot rounds in T at the size of its partial sums, which the
    lift sets (at 24 the fp32 dQ of the zero-valued special channels, sums of K·dS terms near 8192·|dS|
    that cancel, missed the unchanged backward gate on a few elements in 1e5)."""
    f64 = dtype == np.float64
    q0, u, E0 = {(32, False): (3.0, 4, 10), (64, False): (2.0, 8, 10), (96, False): (3.0, 8, 9), (128, False): (3.0, 8, 9),
                (256, False): (2.0, 16, 9), (300, False): (2.5, 16, 8),
                (32, True): (2.0, 16, 9), (64, True): (3.0, 16, 8), (128, True): (2.0, 32, 8),
                (256, True): (3.0, 32, 7), (300, True): (3.0, 32, 7)}[(d, f64)]
    lift = 24.0 if dtype == np.float16 else 4.0
    q0, u, E0 = (q0, 2 * u, E0 - 1) if big else (q0, u, E0)
    return Ramp(W, q0, u, E0 if E is None else E, lift=lift)


def _c(id, dtype, policy, mode, d, vd, qs, ks, W, tile, big=False, E=None, **kw):
    if isinstance(qs, int):
        qs, ks = (qs,), (ks,)
    return Case(id, dtype, policy, mode, d, vd, qs, ks, _ramp(d, W, dtype, big, E), tile, **kw)


F16, F32, F64 = np.float16, np.float32, np.float64
# nk = 64·12 + 8 = 776 where the 16-byte staging needs nk % 8 == 0, 64·12 + 5 = 773 for the element-wise
# one: 13 plateaus with a ragged last one.  Routes are worked out from fwd_f16_choice (fa_fwd_f16_choice.h),
# fwd_f16_band_positions (fa_fwd_f16_band.hip), launch_fwd_f32 (fa_fwd_f32.hip) and launch_fwd_f64 (fa_f64.hip).  fp16
# cases carry bwd=True only where the emulated deviation passes the backward gate at half the allowance
# (profiles/score_ramp_gate.txt).
CASES = [
    # ---- fp16, product library
    # fwd_f16_pingpong_kernel: d <= 64, full policy, nk % 8 == 0
    _c("f16-pingpong-d64-full", F16, "full", "none_front", 64, 64, 300, 776, 64, 64),
    # fwd_f16_fast_kernel<64, 8, POL 1>: causal is an interval rule, not a 1d local one -> the 8-wave kernel
    _c("f16-8wave-d64-causal", F16, "causal", "none_front", 64, 64, 776, 776, 64, 64),
    _c("f16-8wave-d64-causal-big", F16, "causal", "scale_end", 64, 64, 300, 776, 64, 64, big=True),
    # fwd_f16_fast_kernel<64, 4, POL 1>: 1d local, v_d = 48 != 64 so fwd_f16_band_positions declines
    _c("f16-4wave-d64-local", F16, "local", "none_front", 64, 48, 1000, 1000, 64, 64, ws=100),
    # fwd_f16_band_kernel: 1d local, ls = 0, d = v_d = 64, nq % 8 == nk % 8 == 0
    _c("f16-band-local", F16, "local", "none_front", 64, 64, 1000, 1000, 64, 64, ws=100),
    _c("f16-band-local-causal", F16, "local", "none_front", 64, 64, 1000, 1000, 64, 64, ws=100, causal=True,
       big=True),
    # fwd_f16_gap128_kernel<0> / <1>: 64 < d <= 128, full and interval rules, nq past one 256-query block
    _c("f16-gap128-full", F16, "full", "none_front", 128, 128, 300, 776, 64, 64),
    _c("f16-gap128-causal", F16, "causal", "none_front", 128, 128, 776, 776, 64, 64),
    # fwd_f16_fast_kernel<128, 4, POL 1>: local windows keep the 4-wave blocks at d = 128
    _c("f16-4wave-d128-local", F16, "local", "none_front", 128, 128, 1000, 1000, 64, 64, ws=100, big=True),
    # fwd_f16_wide_kernel<POL, ALN>: 128 < d <= 256; <0, true>, <1, true>, <0, false>, <2, false>
    _c("f16-wide-full", F16, "full", "none_front", 256, 256, 300, 776, 64, 64),
    _c("f16-wide-causal", F16, "causal", "none_front", 256, 256, 776, 776, 64, 64),
    _c("f16-wide-full-elem", F16, "full", "none_front", 256, 256, 300, 773, 64, 64),
    _c("f16-wide-strided-elem", F16, "local", "none_front", 256, 256, 773, 773, 64, 64, ws=60, ls=2, big=True),
    # fwd_f16_kernel<32, 4, 0, FAST>: max(d, v_d) <= 32 is below the tuned kernels
    _c("f16-core-d32-full", F16, "full", "none_front", 32, 32, 300, 776, 64, 64),
    # fwd_f16_kernel<64, 8, 0, elem> and <128, 4, 1, elem>: nk % 8 != 0
    _c("f16-core-d64-full-elem", F16, "full", "none_front", 64, 64, 300, 773, 64, 64),
    _c("f16-core-d128-causal-elem", F16, "causal", "none_front", 128, 128, 773, 773, 64, 64),
    # fwd_f16_kernel<64, 4, 2, FAST>: a 2d window is no interval rule
    _c("f16-core-d64-local2d", F16, "local", "none_front", 64, 64, (28, 28), (28, 28), 64, 64, ws=9, big=True),
    # ---- fp16, split-key forward (splitk_partial_kernel + splitk_merge_kernel): plateaus of two tiles,
    # so no two consecutive tiles can rebase (waived); whole chunks underflow against the merged max
    *[_c(f"f16-splitk-d{d}-{pol}-nq{nq}", F16, pol, mode, d, d, nq, 2312, 128, 64, split=True,
         waive=("consecutive",))
      for d in (64, 128) for pol, mode in (("full", "none_front"), ("causal", "scale_end")) for nq in (33, 128)],
    # ---- fp32: fwd_f32_kernel<32 / 64 / 128> (64-key tiles), fa_fwd_f32_wide.hip (D = 256, 32-key tiles); the
    # full policy only: elsewhere a row's top products reach σ0·2^E and fp32 rounds its scores at 1e-4
    _c("f32-d32-full", F32, "full", "none_front", 32, 32, 300, 773, 64, 64),
    _c("f32-d64-full", F32, "full", "none_front", 64, 64, 300, 776, 64, 64),
    _c("f32-d128-full", F32, "full", "none_front", 128, 128, 300, 773, 64, 64),
    _c("f32-wide-d256-full", F32, "full", "none_front", 256, 256, 300, 389, 32, 32),
    # the interval-rule instances (POL 1, rule-mixed diagonal tiles) with E = 4: a row's top products stay
    # at or below 16·σ0, which fp32 rounds at 3e-6, and the steps stop at 8σ0 (no exp2 overflow: waived).
    # Forward only.  Under causal every row has most of its P on keys where K[3] = -16u, so the climb rows'
    # dQ[3] is -16u·Σ_k dS = 0 formed from terms of 16u·|dS|, and D = rowsum(dO·O) enters every term: with the
    # kernel's O (a d-term fp32 accumulation, ~10 eps) its error, ~2e-5, is multiplied by 16u·scale and
    # reached 1.04 and 1.53 of the backward allowance on 1 and 5 elements in 1e5 (the gate's rounding scale
    # takes O as rounded once).  The fp32 backward is checked on the four full-policy cases above.
    _c("f32-d64-causal-e4", F32, "causal", "none_front", 64, 64, 773, 773, 64, 64, E=4, bwd=False,
       waive=("overflow",)),
    _c("f32-wide-d256-causal-e4", F32, "causal", "none_front", 256, 256, 389, 389, 32, 32, E=4, bwd=False,
       waive=("overflow",)),
    # ---- fp64: fwd_f64_kernel<D, POL, NW, TT>, TT = 32 keys up to 128 channels, 16 at D = 256
    _c("f64-d32-full", F64, "full", "none_front", 32, 32, 300, 389, 32, 32),
    _c("f64-d64-causal", F64, "causal", "none_front", 64, 64, 389, 389, 32, 32),
    _c("f64-d64-full-w16", F64, "full", "none_front", 64, 64, 150, 213, 16, 32),
    _c("f64-d128-full", F64, "full", "none_front", 128, 128, 300, 389, 32, 32),
    _c("f64-d256-full-w16", F64, "full", "none_front", 256, 256, 150, 197, 16, 16),
    _c("f64-d256-causal-w16", F64, "causal", "none_front", 256, 256, 197, 197, 16, 16),
    # ---- past 256 channels: the SIMT kernels (fa_generic.hip) move m on every tile; the model's tile and
    # threshold are nominal there and show only that the staircase is in the inputs
    _c("f16-simt-d300", F16, "full", "none_front", 300, 300, 150, 389, 32, 32),
    _c("f32-simt-d300", F32, "full", "none_front", 300, 300, 150, 389, 32, 32),
    _c("f64-simt-d300", F64, "full", "none_front", 300, 300, 150, 389, 32, 32),
    # ---- fp16, diagnostic library: one full-policy climb case per forced structure
    _c("diag-2000-pp", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="2000", bwd=False),
    _c("diag-2200-pingpong", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="2200", bwd=False),
    _c("diag-1814-8wave", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="1814", bwd=False),
    _c("diag-2600-gap", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="2600", bwd=False),
    _c("diag-146-4wave", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="146", bwd=False),
    _c("diag-2700-gap128", F16, "full", "none_front", 128, 128, 300, 776, 64, 64, variant="2700", bwd=False),
    _c("diag-2301-pingpong128", F16, "full", "none_front", 128, 128, 300, 776, 64, 64, variant="2301", bwd=False),
]
CASE_BY_ID = {c.id: c for c in CASES}
# FA_FWD_VARIANT=2116: the ping-pong study kernel without its rebase (kANoRebase); this case must FAIL there
NO_REBASE_CASE = _c("diag-2116-no-rebase", F16, "full", "none_front", 64, 64, 300, 776, 64, 64, variant="2116",
                    bwd=False)


# --------------------------------------------------------------------------- the few-query decode forwards
# fa_forward_ragged / fa_forward_paged / fa_forward_grouped (csrc/fa_fwd_f16_decode.hip, _gqa.hip): one
# workgroup per (K/V slice, key chunk) folds the g heads of the slice into rows rho = head * pitch + query, wave w
# holds rows [32 w, 32 w + 32), every chunk seeds afresh from its first 64-key tile, and a merge kernel weighs the
# chunks by 2^(m_chunk - max).  The K/V slice s attends its first L_s keys, so its staircase is that of a problem
# with L_s keys under ragged_ref.ragged_mask, embedded into capacity-wide K / V.  Past L_s the special channels are
# K[0] = K[3] = 0, K[1] = K[4] = 1 (a climb or fall row's score there lies σ0·2^e(top) ABOVE its top), the lift
# channel continues and V is 65504: a row max, a rebase decision or a PV term taken from a key past the length
# misses the gate by orders of magnitude.
DECODE_TILE, DECODE_THR = 64, 8.0


def decode_plan(nq, cap, g):
    """(chunks, chunk, pitch) of the fused plan over keys [0, cap): the arithmetic tests/test_grouped_plan.py and
    tests/test_ragged_plan.py hold the library to."""
    from tests.test_grouped_plan import _chunks
    pitch = 1
    while pitch < nq:
        pitch *= 2
    chunks, chunk = _chunks(0, cap, g * pitch)
    return chunks, chunk, pitch


@dataclass
class DecodeCase:
    """One staircase case of the decode family.  lens: one length per K/V slice (grouped: every slice has the
    capacity).  tail: the tail-causal form (grouped: the causal rule under scale_end, the same mask at L = cap).
    lift < 0: the sign is carried by Q[2]."""
    id: str
    entry: str                 # "ragged", "paged" (the same inputs through a block table) or "grouped"
    d: int
    vd: int
    g: int
    nq: int
    cap: int
    lens: tuple
    tail: bool = False         # grouped: the causal rule under scale_end
    big: bool = False
    lift: float = 24.0
    pages: tuple = ()          # paged: the page sizes the case runs at
    W: int = 64                # keys a plateau
    seed: int = 0
    waive: tuple = field(default_factory=tuple)

    @property
    def plan(self):
        return decode_plan(self.nq, self.cap, self.g)

    @property
    def ramp(self):
        return _ramp(self.d, self.W, np.float16, self.big)

    def mask(self, L):
        """bool [nq, L]: the keys each query sees in a slice of L live keys (grouped, tail: the causal rule under
        scale_end, whose rows top out at evenly spaced keys)."""
        from tests import ragged_ref
        if self.entry == "grouped" and self.tail:
            return O.problem_mask(O.Problem("causal", 1, "scale_end"), (self.nq,), (L,))
        return ragged_ref.ragged_mask(self.nq, L, L, self.tail)


def _past_fill(K, V, L, ramp, rng):
    kappa = K[2, 0]
    K[:, L:] = rng.uniform(-ramp.a, ramp.a, K[:, L:].shape)
    K[2, L:] = kappa
    K[0, L:] = K[3, L:] = 0.0
    K[1, L:] = K[4, L:] = 1.0
    V[:, L:] = 65504.0


def decode_inputs(case):
    """Q [bkv * g, d, nq], K [bkv, d, cap], V [bkv, v_d, cap] (fp16), and per Q slice the row kinds [nq], the info
    dict of ramp_inputs over the slice's L keys (None for L = 0) and the bound of m_rounding_bound [nq]."""
    d, vd, g, nq, cap, ramp = case.d, case.vd, case.g, case.nq, case.cap, case.ramp
    lens = [min(max(int(L), 0), cap) for L in case.lens]
    bkv = len(lens)
    rng = np.random.default_rng(case.seed + 991)
    Q = rng.uniform(-2, 2, (bkv * g, d, nq)).astype(np.float16)
    K = np.zeros((bkv, d, cap), np.float16)
    V = np.zeros((bkv, vd, cap), np.float16)
    Lq, kappa = lift_pair(d, abs(ramp.lift))
    kinds, infos, bound = [], [], np.zeros((bkv * g, nq))
    prob = O.Problem("full", 1, "none_front")
    for s, L in enumerate(lens):
        k64, v64 = np.zeros((d, cap)), np.zeros((vd, cap))
        k64[2] = kappa
        _past_fill(k64, v64, L, ramp, rng)
        mask = case.mask(L) if L else None
        for h in range(g):
            bi = s * g + h
            if L == 0:
                Q[bi, 2] = np.float16(Lq)
                kinds.append(np.full(nq, FLAT)); infos.append(None)
                continue
            (Qh, Kh, Vh, _), info = ramp_inputs(prob, np.float16, (1,), d, vd, (nq,), (L,), ramp, seed=case.seed + 100 * s + h,
                                                mask=mask, row0=h * nq)
            if h == 0:
                k64[:, :L], v64[:, :L] = Kh[0], Vh[0]
                K[s], V[s] = k64, v64
            assert np.array_equal(Kh[0, :N_SPECIAL], K[s, :N_SPECIAL, :L])   # the special channels do not depend on the seed
            Q[bi] = Qh[0]
            kinds.append(info["kind"]); infos.append(info)
            bound[bi] = m_rounding_bound(Qh, K[s:s + 1, :, :L], info, np.float16, d)[0]
        if L == 0:
            K[s], V[s] = k64, v64
    if case.lift < 0:
        Q[:, 2] = -Q[:, 2]
    return dict(Q=Q, K=K, V=V, lens=lens, kinds=kinds, infos=infos, bound=bound)


def decode_chunk_model(case, made):
    """The rebase model per (Q slice, chunk): every chunk seeds afresh from its first tile.  Returns a list of
    dicts (s, h, c, rebased [nq, tiles], active, kind, last: the chunk holds the slice's ragged last tile) and the
    merge weights [(s, h, q, [float32 weight of every chunk that holds a key of the row])]."""
    chunks, chunk, _ = case.plan
    out, weights = [], []
    for bi, info in enumerate(made["infos"]):
        s, h = divmod(bi, case.g)
        L = made["lens"][s]
        if info is None:
            continue
        scores = kernel_scores(made["Q"][bi][None], made["K"][s][None, :, :L], case.d, True)
        mask = info["mask"]
        cmax = []
        for c in range(chunks):
            k0, k1 = c * chunk, min((c + 1) * chunk, L)
            if k0 >= L:
                break
            rebased, active = rebase_tiles(scores[:, k0:k1], mask[:, k0:k1], DECODE_TILE, DECODE_THR)
            out.append(dict(s=s, h=h, c=c, rebased=rebased, active=active, kind=info["kind"],
                            last=(k1 == L and L % DECODE_TILE != 0)))
            cmax.append(np.where(mask[:, k0:k1], scores[:, k0:k1], -np.inf).max(axis=1))
        cmax = np.stack(cmax, axis=1)                               # [nq, live chunks]
        for q in np.nonzero(info["has"])[0]:
            live = np.isfinite(cmax[q])
            weights.append((s, h, int(q), np.exp2(cmax[q, live] - cmax[q, live].max()).astype(np.float32)))
    return out, weights


def decode_conditions(case, made):
    """The conditions a decode case must meet (tests/test_decode_score_ramp_inputs.py), as a dict of booleans."""
    per_chunk, weights = decode_chunk_model(case, made)
    _, _, pitch = case.plan
    cond = dict(consecutive=False, last=False, quiet=False, others_still=True, n=0, waves_hold_a_still_row=True,
                fired_waves=0, idle=False)
    fired = {}                                                       # (s, c) -> bool [g * pitch]: the row rebased
    still = {}                                                       # (s, c) -> bool [g * pitch]: must not move
    for r in per_chunk:
        c = rebase_conditions(r["rebased"], r["active"], r["kind"])
        cond["consecutive"] |= c["consecutive"]
        cond["quiet"] |= c["quiet"]
        cond["last"] |= c["last"] and r["last"]
        cond["others_still"] &= c["others_still"]
        cond["n"] += c["n"]
        key = (r["s"], r["c"])
        f = fired.setdefault(key, np.zeros(case.g * pitch, bool))
        st = still.setdefault(key, np.ones(case.g * pitch, bool))  # padding rows and the rows of absent heads stay
        rows = r["h"] * pitch + np.arange(case.nq)
        f[rows] = r["rebased"].any(axis=1)
        st[rows] = (r["kind"] != CLIMB) | ~r["active"].any(axis=1)
        # a row without an allowed key in a tile on which a wave-mate rebases (never seeded, or the tile is masked)
        for w in range(0, case.nq, 32) if pitch > 32 else [0]:
            rows_w = slice(w, w + 32) if pitch > 32 else slice(0, case.nq)
            tiles = r["rebased"][rows_w].any(axis=0)
            cond["idle"] |= bool((~r["active"][rows_w][:, tiles]).any())
    for key, f in fired.items():
        assert not (f & still[key]).any()
        for w in range(0, case.g * pitch, 32):
            if f[w:w + 32].any():
                cond["fired_waves"] += 1
                cond["waves_hold_a_still_row"] &= bool(still[key][w:w + 32].any())
    ws = np.concatenate([w[3] for w in weights if w[3].size >= 2] or [np.ones(1, np.float32)])
    cond["merge_zero"] = bool((ws == 0).any())
    cond["merge_between"] = bool(((ws > 0) & (ws < 1)).any())
    return cond


def emulate_ragged_f16(Q, K, V, kv_lens, g, tail):
    """emulate_f16's forward over the ragged rule: (O fp16 [b, v_d, nq], l f32 [b, nq], m fp16 [b, nq]) with the
    documented roundings and, for the rows without a key, O = 0, l = 0 and m = bytes 0xFA as the kernels store."""
    from tests import ragged_ref
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    c2 = np.float32(np.float32(1.0 / math.sqrt(d)) * np.float32(LOG2E))
    o = np.zeros((b, vd, nq), np.float16)
    l = np.zeros((b, nq), np.float32)
    m = np.full((b, nq), 0xFAFA, np.uint16).view(np.float16)
    for i in range(b):
        L = min(max(int(kv_lens[i // g]), 0), cap)
        mask = ragged_ref.ragged_mask(nq, cap, L, tail)[:, :L]
        has = mask.any(axis=1)
        if not has.any():
            continue
        qs16 = (Q[i].astype(np.float32) * c2).astype(np.float16).astype(np.float64)
        k, v = K[i // g][:, :L].astype(np.float64), V[i // g][:, :L].astype(np.float64)
        s2 = np.where(mask, qs16.T @ k, -np.inf)
        m2 = np.where(has, s2.max(axis=1), 0.0)
        p16 = np.exp2(s2 - m2[:, None]).astype(np.float16).astype(np.float64)
        l_run = np.where(has, p16.sum(axis=1), 1.0)
        o16 = ((v @ p16.T) / l_run).astype(np.float16)
        m16 = (m2 / LOG2E).astype(np.float16)
        l32 = (l_run * np.exp2(m2 - m16.astype(np.float64) * LOG2E)).astype(np.float32)
        o[i][:, has], l[i][has], m[i][has] = o16[:, has], l32[has], m16[has]
    return o, l, m


def kv8_split(k_scale):
    """(e, r) with k_scale = 2^e * r as kv8_mul (csrc/fa_fwd_f16_fewq.h) splits the float32 scale: e = round(log2)
    clamped to [-8, 7] from the scale's bits, r the exact float32 quotient."""
    kb = int(np.float32(k_scale).view(np.uint32))
    e = (kb >> 23) - 127 + (1 if (kb & 0x7FFFFF) >= 0x3504F3 else 0)
    e = min(max(e, -8), 7)
    return e, np.float32(np.float32(k_scale) * np.float32(2.0 ** -e))


def emulate_cache_f16(Q, K, V, kv_lens, g, tail, window=0, k_scale=None, v_scale=None, hk=1):
    """emulate_ragged_f16 with a sliding window (window >= 1: tests/window_ref.window_mask in place of the ragged
    mask) and / or an FP8 cache (K, V uint8: e4m3fn bytes; k_scale / v_scale float32 [hk] or None for 1.0, K/V slice
    s being head s % hk) with the documented split: Q' = fp16(q * (c2 * r)) with the product c2 * r in fp32,
    K' = k8 * 2^e (exact in fp16) and v_scale multiplying the accumulator.  Only the keys from the first to the
    last one that some query sees are read."""
    from tests import fp8_ref, ragged_ref, window_ref
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    fp8 = K.dtype == np.uint8
    c2 = np.float32(np.float32(1.0 / math.sqrt(d)) * np.float32(LOG2E))
    o = np.zeros((b, vd, nq), np.float16)
    l = np.zeros((b, nq), np.float32)
    m = np.full((b, nq), 0xFAFA, np.uint16).view(np.float16)
    for i in range(b):
        s = i // g
        L = min(max(int(kv_lens[s]), 0), cap)
        mask = window_ref.window_mask(nq, cap, L, window) if window else ragged_ref.ragged_mask(nq, cap, L, tail)
        has = mask.any(axis=1)
        if not has.any():
            continue
        cols = np.nonzero(mask.any(axis=0))[0]
        j0, j1 = int(cols[0]), int(cols[-1]) + 1
        mask = mask[:, j0:j1]
        e, r = kv8_split(1.0 if k_scale is None else k_scale[s % hk]) if fp8 else (0, np.float32(1.0))
        vmul = float(np.float32(v_scale[s % hk])) if fp8 and v_scale is not None else 1.0
        qs16 = (Q[i].astype(np.float32) * np.float32(c2 * r)).astype(np.float16).astype(np.float64)
        if fp8:
            k = (fp8_ref.decode(K[s][:, j0:j1]) * 2.0 ** e).astype(np.float16).astype(np.float64)
            v = fp8_ref.decode(V[s][:, j0:j1])
        else:
            k, v = K[s][:, j0:j1].astype(np.float64), V[s][:, j0:j1].astype(np.float64)
        s2 = np.where(mask, qs16.T @ k, -np.inf)
        m2 = np.where(has, s2.max(axis=1), 0.0)
        p16 = np.exp2(s2 - m2[:, None]).astype(np.float16).astype(np.float64)
        l_run = np.where(has, p16.sum(axis=1), 1.0)
        o16 = ((v @ p16.T) * vmul / l_run).astype(np.float16)
        m16 = (m2 / LOG2E).astype(np.float16)
        l32 = (l_run * np.exp2(m2 - m16.astype(np.float64) * LOG2E)).astype(np.float32)
        o[i][:, has], l[i][has], m[i][has] = o16[:, has], l32[has], m16[has]
    return o, l, m


# The decode cases.  Plateaus of one 64-key tile.  Chunks are 512 keys up to 64 folded rows and 1024 above (g = 2,
# nq = 33: pitch 64, 128 rows), so three chunks need a capacity past 1024 / 2048 keys.  Each case holds, in ONE call:
#   c2 + 148  a length that ends mid-tile with three live tiles in the last chunk (e = 2, 1, 0: the seed, a quiet 2σ0
#             step and the ragged last tile's σ0 step, which rebases because 3σ0 has accumulated); in the chunk before
#             it every tile after the first steps by >= 4σ0 (consecutive rebases), and chunk 0 is one level (quiet);
#   c2        a length exactly on the edge of chunk 2;
#   c2 + 1    one key past it: the top plateau's only key sits alone in its chunk, chunk 1 ends σ0 under it (a merge
#             weight strictly between 0 and 1) and chunk 0 more than 500σ0 (weight exactly 0 in fp32);
#   40        under one tile;   0  no key;   and under the tail rule
#   nq - 1    row 0 never seeds while the seed tile moves its wave-mates' m_run by the lift (a row without any key has
#             L - nq + i < 0, so a wave-mate within 32 rows tops out below key 32: no later tile can rebase beside it);
#   c2 + 132  only the last four queries see the last tile's four keys; the climb rows among them rebase there (3σ0
#             accumulated) while that tile is masked for the other rows of their wave ("idle": asserted for the tail
#             cases; under the full form every row of a slice sees every live key).
# (c2 = 2 * chunk.)
def _d(id, entry, d, vd, g, nq, cap, tail=False, lens=None, **kw):
    chunk = decode_plan(nq, cap, g)[1]
    if lens is None:
        lens = (2 * chunk + 148, 2 * chunk, 2 * chunk + 1, 40, 0) + ((nq - 1, 2 * chunk + 132) if tail else ())
    return DecodeCase(id, entry, d, vd, g, nq, cap, tuple(lens), tail, **kw)


DECODE_CASES = [
    # ---- fa_forward_ragged, full form, 16-byte staging (decode_partial_kernel<RaggedCache, D, 0, true> + ragged_merge_kernel);
    # the d = 64 case runs through fa_forward_paged as well (the same kernel over PagedCache, pages of 64 and 192 keys)
    _d("ragged-d64-g4q4-full", "ragged", 64, 64, 4, 4, 1344, pages=(64, 192)),
    _d("ragged-d128-g2q33-full", "ragged", 128, 128, 2, 33, 2568),     # pitch 64: a wave holds a run of one head's queries
    _d("ragged-d32-g8q1-full", "ragged", 32, 32, 8, 1, 1336),         # decode: eight heads side by side in one wave
    # ---- element-wise staging (capacity % 8 != 0, d != v_d): decode_partial_kernel<RaggedCache, 128, 0, false>
    _d("ragged-d96v40-g3q3-elem", "ragged", 96, 40, 3, 3, 1341),
    # ---- tail-causal: decode_partial_kernel<RaggedCache, D, 1, .> through RaggedRows::lane_interval
    _d("ragged-d64-g2q16-tail", "ragged", 64, 64, 2, 16, 1344, tail=True, pages=(64, 192)),
    _d("ragged-d128-g1q33-tail", "ragged", 128, 128, 1, 33, 1336, tail=True),
    # the doubled σ0 where the rows' tops differ: at c2 + 1, + 65 and + 129 the window of the last 16 keys lies across
    # a plateau edge, so rows 0 .. 14 top out one plateau (2σ0 > 8: a rebase of their own) below row 15.  The last
    # tile's step alone (σ0 <= 8) never fires, and every row sees the tile before it: "idle" waived.  Capacity % 8 != 0:
    # the tail rule with element-wise staging at d = v_d = 64
    _d("ragged-d64-g2q16-tail-big", "ragged", 64, 64, 2, 16, 1341, tail=True, big=True,
       lens=(1025, 1089, 1153, 1172, 1024, 40, 0, 15), waive=("idle",)),
    # 128 queries of one head, plateaus of 16 keys: L = 127 leaves row 0 without a key and rows 1 .. 64 without one in
    # the second tile while the rows past 64 step up by 15σ0 there.  One chunk: nothing to merge, no quiet stretch
    DecodeCase("ragged-d64-g1q128-tail-w16", "ragged", 64, 64, 1, 128, 1344, (127, 128, 0), True, W=16,
               waive=("consecutive", "quiet", "merge")),
    # ---- the lift negated: every score lies far below m_run's initial 0, the seed moves down, the stored m is negative
    _d("ragged-d64-g4q4-full-neglift", "ragged", 64, 64, 4, 4, 1344, lift=-24.0),
    # ---- fa_forward_grouped (gqa_partial_kernel + gqa_merge_kernel): every slice has the capacity, c2 + 136 / + 141
    # keys.  nq = 7 and 3: under the causal rule only the last query reaches the ragged last tile, and folded row
    # 0 * nq + nq - 1 is then a climb row
    _d("grouped-d128-g4q7-full", "grouped", 128, 128, 4, 7, 1160, lens=(1160, 1160)),
    _d("grouped-d128-g4q7-causal", "grouped", 128, 128, 4, 7, 1160, tail=True, lens=(1160, 1160)),
    _d("grouped-d32-g8q3-full-elem", "grouped", 32, 32, 8, 3, 1165, lens=(1165, 1165)),
    _d("grouped-d32-g8q3-causal-elem", "grouped", 32, 32, 8, 3, 1165, tail=True, lens=(1165, 1165)),
]
DECODE_CASE_BY_ID = {c.id: c for c in DECODE_CASES}


def windowed_tail_cases():
    """The tail cases whose lengths all lie below the capacity: at W = capacity - 1 the sliding-window forwards run
    them un-delegated under the tail plan and the tail mask (tests/test_gpu_decode_score_range.py)."""
    return [c for c in DECODE_CASES if c.entry == "ragged" and c.tail and max(c.lens) < c.cap]


def window_capacity(case, page=0):
    """the capacity a windowed run of ``case`` uses: its own, or for a paged run that rounded up to the page"""
    return -(-case.cap // page) * page if page else case.cap
