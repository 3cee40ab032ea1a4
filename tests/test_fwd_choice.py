"""CPU tests of the forward's kernel choice (csrc/fa_fwd_f16_choice.h through fa_forward_kernel).
Host-only: the pointers are made-up addresses of which the library reads the alignment, nothing is allocated and
nothing is launched.  TABLE is also what tools/dispatch_trace.py runs on a device, row by row."""

import ctypes
import itertools
import re

import pytest

from tf_flash_attention_amd import _lib

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}
BASE = 1 << 20  # a made-up, 16-byte aligned address


def problem(policy="full", qs=(256,), ks=(256,), d=64, vd=None, mode="none_front", dtype=_lib.F16, b=2, ws=1, ls=0,
            causal=False, **_):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], b, qs, ks, d, d if vd is None else vd, ws, ls,
                             causal)


def kernel_name(p, off=(0, 0, 0)):
    """What fa_forward would launch for problem p with Q, K, V at BASE + off bytes."""
    q, k, v = (ctypes.c_void_p(BASE + o) for o in off)
    return _lib.lib().fa_forward_kernel(ctypes.byref(p), q, k, v).decode()


def G(d, nw, pol, aligned, f=8):
    return f"fwd_f16_kernel<{d}, {nw}, {pol}, {'true' if aligned else 'false'}, {f}>"


def W(pol, aligned):
    return f"fwd_f16_wide_kernel<{pol}, {'true' if aligned else 'false'}>"


PINGPONG = "fwd_f16_pingpong_kernel"
GAP128_FULL, GAP128_RULE = "fwd_f16_gap128_kernel<0, 0>", "fwd_f16_gap128_kernel<1, 0>"
FAST_64_8, FAST_64_4, FAST_128_4 = (f"fwd_f16_fast_kernel<{x}>" for x in ("64, 8, 1, 14", "64, 4, 1, 6", "128, 4, 1, 6"))
BAND = {t: f"fwd_f16_band_kernel<{t}>" for t in (9, 13, 17, 21)}

# (id, problem keywords [off: byte offsets of Q, K, V], the kernel), worked out from the dispatch order of
# launch_fwd_f16 / launch_fwd_f16_fast and the fwd_f16_*_supported predicates as they stood before the choice function
TABLE = [
    # ---- the tuned kernels, one row a leaf
    ("pingpong", dict(), PINGPONG),
    ("pingpong-d40-vd64", dict(d=40, vd=64), PINGPONG),
    ("pingpong-d33", dict(d=33, qs=(72,), ks=(136,)), PINGPONG),
    ("pingpong-vd-narrow", dict(d=64, vd=8), PINGPONG),
    ("pingpong-2d", dict(qs=(8, 32), ks=(16, 16)), PINGPONG),
    ("gap128-full", dict(d=128), GAP128_FULL),
    ("gap128-full-d65-vd72", dict(d=65, vd=72), GAP128_FULL),
    ("gap128-causal", dict(policy="causal", d=128), GAP128_RULE),
    ("gap128-causal-vd-narrow", dict(policy="causal", d=128, vd=16, mode="scale_end"), GAP128_RULE),
    ("fast-64-8-causal", dict(policy="causal"), FAST_64_8),
    ("fast-64-8-causal-d33", dict(policy="causal", d=33, vd=40, qs=(72,), ks=(264,), mode="scale_front"), FAST_64_8),
    ("fast-128-4-local", dict(policy="local", d=128, ws=64), FAST_128_4),
    ("fast-128-4-local-causal", dict(policy="local", d=96, vd=128, ws=64, causal=True), FAST_128_4),
    ("band-9", dict(policy="local", qs=(1024,), ks=(1024,), ws=64), BAND[9]),
    ("band-9-d40", dict(policy="local", qs=(1024,), ks=(1024,), d=40, vd=64, ws=16, causal=True), BAND[9]),
    ("band-13", dict(policy="local", qs=(2048,), ks=(2048,), ws=384), BAND[13]),
    ("band-17", dict(policy="local", qs=(2048,), ks=(2048,), ws=512), BAND[17]),
    ("band-21", dict(policy="local", qs=(2048,), ks=(2048,), ws=640), BAND[21]),
    # ---- the general kernel's four instances
    ("general-32", dict(d=32), G(32, 4, 0, True)),
    ("general-32-d16", dict(d=16, vd=32, policy="causal"), G(32, 4, 1, False)),
    ("general-64-4-strided", dict(policy="local", qs=(512,), ks=(512,), ws=16, ls=1), G(64, 4, 2, True)),
    ("general-64-8-nk100", dict(ks=(100,)), G(64, 8, 0, False)),
    ("general-128-4-nk100", dict(d=128, ks=(100,), policy="causal"), G(128, 4, 1, False)),
    # ---- the wide kernel: aligned or not under each POL
    ("wide-full", dict(d=256), W(0, True)),
    ("wide-causal", dict(d=129, vd=64, policy="causal"), W(1, True)),
    ("wide-local-1d", dict(d=64, vd=200, policy="local", ws=16), W(1, True)),
    ("wide-local-2d", dict(d=256, policy="local", qs=(16, 16), ks=(16, 16), ws=4), W(2, True)),
    ("wide-full-nk100", dict(d=256, ks=(100,)), W(0, False)),
    ("wide-causal-k-off", dict(d=192, policy="causal", off=(0, 8, 0)), W(1, False)),
    ("wide-strided-v-off", dict(d=256, policy="local", ws=4, ls=2, off=(0, 0, 2)), W(2, False)),
    # ---- why a tuned kernel is refused, one row a reason
    ("refuse-nk-not-8", dict(ks=(260,)), G(64, 8, 0, False)),
    ("refuse-nk-not-8-d128", dict(d=128, ks=(260,)), G(128, 4, 0, False)),
    ("refuse-k-off", dict(off=(0, 8, 0)), G(64, 8, 0, False)),
    ("refuse-v-off", dict(d=128, policy="causal", off=(0, 0, 2)), G(128, 4, 1, False)),
    ("refuse-k-off-d48", dict(d=48, off=(0, 2, 0)), G(64, 8, 0, False)),
    ("q-off-is-no-reason", dict(off=(2, 0, 0)), PINGPONG),
    ("band-refuse-q-off", dict(policy="local", qs=(1024,), ks=(1024,), ws=64, off=(8, 0, 0)), FAST_64_4),
    ("band-refuse-nq-not-8", dict(policy="local", qs=(1020,), ks=(1024,), ws=64), FAST_64_4),
    ("band-refuse-vd48", dict(policy="local", qs=(1024,), ks=(1024,), vd=48, ws=64), FAST_64_4),
    ("band-refuse-wide-window", dict(policy="local", qs=(4096,), ks=(4096,), ws=1024), FAST_64_4),
    ("refuse-strided-window", dict(policy="local", qs=(1024,), ks=(1024,), ws=16, ls=1), G(64, 4, 2, True)),
    ("refuse-strided-window-d128", dict(policy="local", d=128, qs=(1024,), ks=(1024,), ws=16, ls=2), G(128, 4, 2, True)),
    ("refuse-2d-window", dict(policy="local", qs=(32, 32), ks=(32, 32), ws=4), G(64, 4, 2, True)),
    ("refuse-2d-window-d128", dict(policy="local", d=128, qs=(32, 32), ks=(32, 32), ws=4), G(128, 4, 2, True)),
    ("refuse-d32", dict(d=32, vd=32, policy="causal"), G(32, 4, 1, True)),
    ("refuse-d8-local", dict(d=8, vd=24, policy="local", ws=16), G(32, 4, 1, False)),
    # ---- the other paths and nothing at all
    ("fp32", dict(dtype=_lib.F32), "fwd_f32"),
    ("fp64", dict(dtype=_lib.F64), "fwd_f64"),
    ("fp16-d257", dict(d=257), "fwd_generic"),
    ("fp32-d300", dict(dtype=_lib.F32, d=300), "fwd_generic"),
    ("empty-batch", dict(b=0), "none"),
    ("no-queries", dict(qs=(0,)), "none"),
    ("invalid", dict(d=0), "none"),
    ("too-many-channels", dict(d=70000), "none"),
    # ---- the 32-bit limits: a grid of 2^31 workgroups, a slice of 2^31 bytes
    ("grid-last", dict(qs=(128,), b=2**31 - 1), PINGPONG),
    ("grid-over", dict(qs=(128,), b=2**31), "none"),
    ("grid-over-2-blocks", dict(qs=(129,), b=2**30), "none"),
    ("grid-last-wide", dict(d=256, qs=(256,), b=2**30 - 1), W(0, True)),
    ("grid-over-wide", dict(d=256, qs=(256,), b=2**30), "none"),
    ("batch-2^62", dict(qs=(1024,), b=2**62), "none"),
    ("k-slice-last", dict(d=128, qs=(64,), ks=(2**23 - 8,)), GAP128_FULL),
    ("k-slice-over", dict(d=128, qs=(64,), ks=(2**23,)), G(128, 4, 0, True)),
    ("q-slice-over", dict(policy="causal", qs=(2**24,), ks=(64,)), G(64, 8, 1, True)),
    ("k-slice-last-wide", dict(d=256, qs=(64,), ks=(2**22 - 16,)), W(0, True)),
    ("k-slice-over-wide", dict(d=256, qs=(64,), ks=(2**22 - 8,)), "fwd_generic"),
]


@pytest.mark.parametrize("name,kw,want", TABLE, ids=[r[0] for r in TABLE])
def test_table(name, kw, want):
    assert kernel_name(problem(**kw), kw.get("off", (0, 0, 0))) == want


def test_table_covers_every_leaf():
    named = {r[2] for r in TABLE}
    assert {PINGPONG, GAP128_FULL, GAP128_RULE, FAST_64_8, FAST_64_4, FAST_128_4, *BAND.values()} <= named
    assert {W(p, a) for p in range(3) for a in (True, False)} <= named
    general = {re.match(r"fwd_f16_kernel<(\d+, \d+),", n).group(1) for n in named if n.startswith("fwd_f16_kernel<")}
    assert general == {"32, 4", "64, 4", "64, 8", "128, 4"}


KNOWN = ({PINGPONG, GAP128_FULL, GAP128_RULE, FAST_64_8, FAST_64_4, FAST_128_4, *BAND.values()}
         | {W(p, a) for p in range(3) for a in (True, False)}
         | {G(d, nw, p, a) for d, nw in ((32, 4), (64, 4), (64, 8), (128, 4)) for p in range(3) for a in (True, False)})
CHANNELS = (16, 32, 33, 64, 65, 128, 129, 256)
LENGTHS = (1, 8, 72, 136, 264, 4096)
OFFSETS = ((0, 0, 0), (0, 8, 0), (2, 0, 2))


def _seq(n, dims):
    return (n,) if dims == 1 else ((n // 8, 8) if n % 8 == 0 else (1, n))


@pytest.mark.parametrize("policy", sorted(POL))
@pytest.mark.parametrize("dims", (1, 2))
@pytest.mark.parametrize("mode", sorted(SYNC))
def test_sweep(policy, dims, mode):
    """Every fp16 problem of the cross product gets a kernel the product library holds, never one that left it,
    and the same one whatever the batch."""
    fn, seen = _lib.lib().fa_forward_kernel, set()
    ptrs = [tuple(ctypes.c_void_p(BASE + o) for o in off) for off in OFFSETS]
    for nq, nk in itertools.product(LENGTHS, LENGTHS):
        p = problem(policy=policy, qs=_seq(nq, dims), ks=_seq(nk, dims), mode=mode, ws=64)
        ref = ctypes.byref(p)
        for d, vd in itertools.product(CHANNELS, CHANNELS):
            p.d, p.v_d = d, vd
            for q, k, v in ptrs:
                names = set()
                for b in (1, 2, 1024):
                    p.b = b
                    names.add(fn(ref, q, k, v))
                assert len(names) == 1, (nq, nk, d, vd, names)
                seen |= names
    seen = {n.decode() for n in seen}
    assert seen <= KNOWN, seen - KNOWN
    assert not any("pingpong128" in n or n.startswith("fwd_f16_fast_kernel") and ", 0, " in n for n in seen)