#!/usr/bin/env python3
"""Compare the decode-family wrappers of tf_flash_attention_amd/flash_attention.py with those of another version of
that file (the parent commit's), on CPU tensors, without a GPU:

    tools/wrapper_parity.py PARENT            (a git revision, or a path to that version's flash_attention.py)
    tools/wrapper_parity.py PARENT --record   (also write PARENT's Part 1 table to tests/golden/wrapper_messages.json)

Part 1, what a call raises: per wrapper one valid call (it ends in the "no CPU kernel" error), every fault its code can
raise, at batch shapes (), (3,) and (2, 3) where the fault is one of shape, and every two faults whose checks are
neighbours, so that a swapped order gives another first error.  Type and whole text are compared.
Part 2, what reaches the library: both modules run every route against a recording stand-in for the library (live
plans, a fixed workspace size, FA_OK), with the device check, the stream handle and torch.cuda.device replaced alike.
The ordered (entry point, arguments) lists and the returned tensors' shape, dtype and contiguity are compared.  ONE
difference is expected and counted, not filtered: where the wide route of paged_1d runs, PARENT asks
fa_forward_paged_wide_plan twice with the same arguments and the working tree once.
The exit status is 1 on any difference, or if a copy of the module with one message altered shows none (self-check)."""
import contextlib
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from tf_flash_attention_amd import _lib, flash_attention as NEW  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wrapper_messages.json")
F16, F8, I32 = torch.float16, torch.float8_e4m3fn, torch.int32
FORWARDS = ("ragged_1d", "ragged_prefill_1d", "ragged_window_prefill_1d", "paged_1d", "paged_prefill_1d",
            "paged_window_prefill_1d", "mla_paged_1d", "mla_paged_prefill_1d")
WRAPPERS = FORWARDS + ("mla_paged_append_1d", "ragged_append_1d", "paged_append_1d")
BATCHES = ((), (3,), (2, 3))


def load(text, name):
    """A version of flash_attention.py as one more submodule of the package."""
    spec = importlib.util.spec_from_loader("tf_flash_attention_amd." + name, loader=None)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    exec(compile(text, name, "exec"), mod.__dict__)
    return mod


def parent_text(src):
    if os.path.exists(src):
        return open(src).read()
    return subprocess.run(["git", "-C", ROOT, "show", src + ":tf_flash_attention_amd/flash_attention.py"], check=True,
                          capture_output=True, text=True).stdout


def z(shape, dtype=F16, device="cpu"):
    return torch.zeros(tuple(shape), dtype=dtype, device=device)


def base(w, b=(3,), nq=2, kv=F16, c=64, hq=4, hk=2, page=64, dev="cpu"):
    """The arguments of a valid call of wrapper ``w`` by name, at batch shape ``b``."""
    mla, append, paged = w.startswith("mla"), "append" in w, "paged" in w
    if mla:
        c, a = 2 * c, {"KV_pool": z((5, 2 * c, page), kv)}
        a.update({"KV_new": z(b + (c, nq))} if append else {"Q": z(b + (16, c, nq)), "v_channels": 64})
    else:
        K, V = ("K_pool", "V_pool") if paged else ("K", "V")
        lead = (5, hk) if paged else b + (hk,)
        a = {K: z(lead + (c, page if paged else 128), kv, dev), V: z(lead + (c // 2, page if paged else 128), kv, dev)}
        a.update({"K_new": z(b + (hk, c, nq), F16, dev), "V_new": z(b + (hk, c // 2, nq), F16, dev)} if append
                 else {"Q": z(b + (hq, c, nq))})
    if paged:
        a["block_table"] = z(b + (2,), I32)
    a["k_lens"] = z(b, I32, dev)
    if "window_prefill" in w:
        a["window_size"] = 16
    return a


def sub(key, fn):
    """Replace the tensor at ``key`` by ``fn`` of it (what an earlier fault of a pair made a non-tensor stays)."""
    return lambda a: a.__setitem__(key, fn(a[key])) if isinstance(a.get(key), torch.Tensor) else None


def put(**kw):
    return lambda a: a.update(kw)


def both(*fs):
    return lambda a: [f(a) for f in fs]


def faults(w, b):
    """[(id, mutation of base()'s dict, whether it is a fault of shape)] in the order of the wrapper's checks."""
    mla, append, paged, ragged = w.startswith("mla"), "append" in w, "paged" in w, w.startswith("ragged")
    K, V = ("KV_pool", "KV_pool") if mla else ("K_pool", "V_pool") if paged else ("K", "V")
    new = "KV_new" if mla else "K_new"
    q = new if append else "Q"
    ks, nscale = ("kv_scale", 1) if mla else ("k_scale", 2)
    fp8 = both(sub(K, lambda x: x.to(F8)), sub(V, lambda x: x.to(F8)))
    one_d = w.endswith("paged_1d") and not mla or w == "ragged_1d"
    out = []

    def add(name, f, shape=False):
        out.append((name, f, shape))
    if "window_prefill" in w:
        add("window_none", put(window_size=None))
    # the shapes of the cache and of Q or the new tokens
    if ragged and not append:
        add("ndims", sub("V", lambda x: x[..., None]))
        add("ndims_lt3", put(Q=z((64, 2)), K=z((64, 128)), V=z((32, 128))))
    if ragged and append:
        add("kv_ndim", sub("V", lambda x: x[0]), True)
        add("kv_agree", sub("V", lambda x: x[..., :-1]), True)
    if paged:
        add("pool_ndim", sub(K, lambda x: x[0]))
    if paged and not mla:
        add("pools_agree", sub(V, lambda x: x[:-1]))
    if paged and not append:
        add("q_ndim", put(Q=z((64, 2))))
    if not append:
        add("channels", sub("Q", lambda x: x[..., :-1, :]), True)
    if ragged and not append:
        add("batch_shapes", sub("V", lambda x: torch.cat([x, x], 0)), True)
        add("kv_seq", sub("V", lambda x: x[..., :-1]))
    if not append and not mla:
        add("heads", sub("Q", lambda x: x[..., :3, :, :]), True)
    if paged:
        add("no_pages", both(sub(K, lambda x: x[:0]), sub(V, lambda x: x[:0])), True)
    if mla and not append:
        for name, v in (("v_channels_type", 64.0), ("v_channels_bool", True), ("v_channels_lt1", 0)):
            add(name, put(v_channels=v))
    if append:
        add("new_not_tensor", put(**{new: 3}))
        add("new_dtype", sub(new, lambda x: x.float()))
        if not mla:
            add("v_new_dtype", sub("V_new", lambda x: x.float()))
        add("new_shape", sub(new, lambda x: x[..., :-1, :]), True)
        add("new_ndim", sub(new, lambda x: x[..., 0]), True)
    # dtypes and scales
    if not append:
        add("q_dtype", sub("Q", lambda x: x.float()))
        add("q_dtype_int", sub("Q", lambda x: x.int()))
    if not mla:
        add("v_not_fp8", sub(K, lambda x: x.to(F8)))
    add("cache_dtype", sub(K, lambda x: x.float()))
    add("scale_no_fp8", put(**{ks: torch.ones(nscale)}))
    add("scale_dtype", both(fp8, put(**{ks: torch.ones(nscale, dtype=torch.float64)})))
    add("scale_not_tensor", both(fp8, put(**{ks: 1.0})))
    add("scale_shape", both(fp8, put(**{ks: torch.ones(nscale + 1)})))
    add("scale_device", both(fp8, put(**{ks: torch.ones(nscale, device="meta")})))
    if not mla:
        add("scale_noncontiguous", both(fp8, put(k_scale=torch.ones(4)[::2])))
        add("v_scale_dtype", both(fp8, put(v_scale=torch.ones(2, dtype=torch.float16))))
        add("v_scale_shape", both(fp8, put(v_scale=torch.ones(2, 1))))
    # the int32 tensors
    ints = (["block_table"] if paged else []) + ["k_lens"] + (["new_lens"] if append else [])
    with_new_lens = put(new_lens=z(b, I32)) if append else put()
    for n in ints:
        add(n + "_dtype", both(with_new_lens, sub(n, lambda x: x.long())))
    add("k_lens_not_tensor", put(k_lens=3))
    for n in ints:
        add(n + "_shape", both(with_new_lens, sub(n, lambda x: x[..., None])), True)
    if paged:
        add("block_table_empty", sub("block_table", lambda x: x[..., :0]), True)
        add("block_table_0d", put(block_table=z((), I32)), True)
    # a tensor on the meta device beside CPU tensors: the "must be on the device of" checks, which stand between the
    # shapes and grad mode
    for n in ints:
        add(n + "_device", both(with_new_lens, sub(n, lambda x: x.to("meta"))))
    if append:
        add("new_device", sub(new, lambda x: x.to("meta")))
        if not mla:
            add("v_device", sub(V, lambda x: x.to("meta")))
    # the mask and the scale of the MLA forward stand before grad mode, the others' window and mask after it
    def masked(*fs):  # (a good mask and the tail rule unless an earlier fault of the pair set them, then ``fs``)
        return both(lambda a: (a.setdefault("draft_mask", z(b + (2, 1), I32)), a.setdefault("tail_causal", True)), *fs)
    mask = [("mask_type", both(put(draft_mask=3), masked()), False),
            ("mask_dtype", masked(sub("draft_mask", lambda x: x.long())), False),
            ("mask_shape", masked(sub("draft_mask", lambda x: x[..., None])), True),
            ("mask_device", masked(sub("draft_mask", lambda x: x.to("meta"))), False),
            ("mask_no_tail", masked(put(tail_causal=False)), False)]
    if w == "mla_paged_prefill_1d":
        out += mask
    if mla and not append:
        for name, v in (("softmax_scale_zero", 0.0), ("softmax_scale_inf", float("inf")), ("softmax_scale_nan", float("nan"))):
            add(name, put(softmax_scale=v))
    add("grad", sub(q, lambda x: x.requires_grad_()))
    add("cache_grad", both(sub(K, lambda x: x.requires_grad_()), sub(q, lambda x: x.detach())))
    if append:
        add("noncontiguous", sub(V, lambda x: x.transpose(-1, -2).contiguous().transpose(-1, -2)))
    if paged:
        add("page", both(sub(K, lambda x: x[..., :32].contiguous()), sub(V, lambda x: x[..., :32].contiguous())))
        add("page_zero", both(sub(K, lambda x: x[..., :0]), sub(V, lambda x: x[..., :0])))
    if mla and not append:
        add("v_channels_above_c", put(v_channels=192))
    if paged:  # (a table of 2^24 + 1 pages that takes no memory)
        add("capacity", sub("block_table", lambda x: z((1,), I32).expand(tuple(x.shape[:-1]) + (2 ** 24 + 1,))))
    if w == "ragged_append_1d":  # (on the meta device: a contiguous cache of 2^30 + 1 keys that takes no memory)
        add("capacity", lambda a: (a.clear(), a.update(base(w, b, dev="meta")), a.update(
            K=torch.empty(b + (2, 64, 2 ** 30 + 1), dtype=F16, device="meta"),
            V=torch.empty(b + (2, 32, 2 ** 30 + 1), dtype=F16, device="meta"))))
    if w == "mla_paged_prefill_1d":
        add("mask_above_128", put(Q=z(b + (16, 128, 129)), draft_mask=z(b + (129, 5), I32), tail_causal=True))
    if one_d or "window_prefill" in w:
        for name, v in (("window_type", 2.0), ("window_bool", True), ("window_lt1", 0)):
            add(name, put(window_size=v))
    if one_d:
        add("window_no_tail", put(window_size=4))
        out += mask
        add("mask_and_window", masked(put(window_size=4)))
    # the library's own answers: a refusal of the plan, a plan without chunks
    if not append:
        add("no_queries", both(sub("Q", lambda x: x[..., :0]), sub("draft_mask", lambda x: x[..., :0, :0])), True)
        if w.endswith("paged_1d") or w == "ragged_1d":  # g * next_pow2(Nq) above the bound of the unblocked forwards
            add("envelope_rows", sub("Q", lambda x: z(tuple(x.shape[:-1]) + (1100,))), True)
        if mla:  # C = 160 is no multiple of 64
            add("envelope_channels", lambda a: a.update({k: v for k, v in base(w, b, c=80).items() if k in ("Q", "KV_pool")}))
        elif w != "paged_1d":  # 256 channels, which only paged_1d's wide route takes
            add("envelope_channels", lambda a: a.update({k: v for k, v in base(w, b, c=256).items() if k in ("Q", K, V)}))
    return out


def cases():
    """[(wrapper, case id, function of a module's wrapper that makes the call)]; the ids are unique in a wrapper."""
    out = []

    def case(w, cid, b, *muts):
        def run(fn):
            a = base(w, b)
            for m in muts:
                m(a)
            return fn(**a)
        out.append((w, cid, run))
    for w in WRAPPERS:
        case(w, "valid", (3,))
        case(w, "valid_0d", ())
        fs = faults(w, (3,))
        for b in BATCHES:
            for name, f, shape in faults(w, b):
                if shape or b == (3,):
                    case(w, name + "@" + "x".join(map(str, b)), b, f)
        for (n1, f1, _), (n2, f2, _) in zip(fs, fs[1:]):
            case(w, n1 + "+" + n2, (3,), f1, f2)
    return out


def outcome(mod, w, run):
    """(exception type name, whole text) of the call; a call that returns is ("returned", "")."""
    try:
        with torch.enable_grad():
            run(getattr(mod, w))
    except Exception as e:  # noqa: BLE001 (whatever the wrapper raises is the observation)
        return type(e).__name__, str(e)
    return "returned", ""


def golden_entries(table):
    """The table as the golden's entries.  A case that gives, word for word, what an earlier case gives (a pair and its
    first fault, one fault at two batch shapes, one shared check through two wrappers) is written as ``same_as`` that
    [wrapper, case]: the text is stored once, the assertion stays."""
    first = {}
    for w, cid, kind, text in table:
        ref = first.setdefault((kind, text), [w, cid])
        yield ({"wrapper": w, "case": cid, "type": kind, "text": text} if ref == [w, cid]
               else {"wrapper": w, "case": cid, "same_as": ref})


def load_golden(path=GOLDEN):
    """{(wrapper, case): (type, text)} of the golden, ``same_as`` entries resolved."""
    with open(path) as f:
        entries = json.load(f)
    full = {(e["wrapper"], e["case"]): (e["type"], e["text"]) for e in entries if "same_as" not in e}
    return {(e["wrapper"], e["case"]): full[tuple(e.get("same_as", (e["wrapper"], e["case"])))] for e in entries}


def part1(mods):
    table = [[(w, cid) + outcome(m, w, run) for w, cid, run in cases()] for m in mods]
    return table, [(a, b) for a, b in zip(*table) if a != b]


class Recorder:
    """Stands in for the library: plans report chunks (but those named in ``dead``), a workspace is 4096 bytes, every
    other call returns FA_OK.  Pointers are recorded as the input they belong to, or as "new"."""

    def __init__(self, inputs, dead=()):
        self.calls, self.dead = [], dead
        self.names = {t.data_ptr(): n for n, t in inputs.items() if isinstance(t, torch.Tensor)}

    def show(self, x):
        if isinstance(x, _lib.FaProblem):
            return tuple(tuple(v) if hasattr(v, "__len__") else v for v in (getattr(x, n) for n, _ in x._fields_))
        if isinstance(x, ctypes.Array):
            return "int32[%d]" % len(x)
        return self.names.get(x, "new") if isinstance(x, int) and x >= 2 ** 32 else x

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name,) + tuple(self.show(x) for x in args))
            if name.endswith("_plan"):
                args[-1][0] = int(name not in self.dead)
            return 4096 if name.endswith("_workspace_bytes") else _lib.FA_OK
        return f


def routes():
    """[(wrapper, route id, arguments, dead plans)] over every route to the library."""
    out = []
    for cache in ("ragged", "paged"):
        for kv, scaled in ((F16, False), (F8, False), (F8, True)):
            sc = dict(k_scale=torch.ones(2), v_scale=torch.ones(2)) if scaled else {}
            tag = "/" + ("f16" if kv is F16 else "fp8_scaled" if scaled else "fp8")
            for form, w, kw in (("plain", "_1d", {}), ("tail", "_1d", dict(tail_causal=True, returning_l_m=True)),
                                ("window", "_1d", dict(tail_causal=True, window_size=5)),
                                ("tree", "_1d", dict(tail_causal=True, draft_mask=torch.ones(3, 2, 1, dtype=I32))),
                                ("prefill", "_prefill_1d", dict(returning_l_m=True)), ("window_prefill", "_window_prefill_1d", {})):
                out.append((cache + w, form + tag, dict(base(cache + w, kv=kv), **sc, **kw), ()))
            for new_lens in (False, True):
                a = dict(base(cache + "_append_1d", kv=kv), **sc, **({"new_lens": z((3,), I32)} if new_lens else {}))
                out.append((cache + "_append_1d", "append" + "_new_lens" * new_lens + tag, a, ()))
    for form, kw, dead in (("wide", {}, ()), ("wide_window", dict(tail_causal=True, window_size=7), ()), ("wide_tail", dict(tail_causal=True), ()),
                           ("wide_refused", {}, ("fa_forward_paged_wide_plan",))):
        out.append(("paged_1d", form, dict(base("paged_1d", c=256), **kw), dead))
    for kv, scaled in ((F16, False), (F8, False), (F8, True)):
        sc = dict(kv_scale=torch.ones(1)) if scaled else {}
        tag = "/" + ("f16" if kv is F16 else "fp8_scaled" if scaled else "fp8")
        for form, w, a in (("decode", "mla_paged_1d", {}), ("unblocked", "mla_paged_prefill_1d", dict(softmax_scale=0.25)),
                           ("blocked", "mla_paged_prefill_1d", dict(Q=z((3, 16, 128, 40)), tail_causal=True, returning_l_m=True)),
                           ("masked", "mla_paged_prefill_1d", dict(tail_causal=True, draft_mask=torch.ones(3, 2, 1, dtype=I32)))):
            out.append((w, form + tag, dict(base(w, kv=kv), **sc, **a), ()))
        for new_lens in (False, True):
            a = dict(base("mla_paged_append_1d", kv=kv), **sc, **({"new_lens": z((3,), I32)} if new_lens else {}))
            out.append(("mla_paged_append_1d", "append" + "_new_lens" * new_lens + tag, a, ()))
    return out


def part2(mods):
    """Per route the two recordings; returns (routes compared, differences, routes with the expected wide difference)."""
    diffs, wide, todo = [], [], routes()
    real = [torch.cuda.device] + [(m._check_device_tensors, m._stream_handle) for m in mods]
    torch.cuda.device = lambda dev: contextlib.nullcontext()
    try:
        for w, rid, args, dead in todo:
            got = []
            for m in mods:
                m._check_device_tensors, m._stream_handle = (lambda *ts: None), (lambda dev: 0)
                _lib._tls.override = rec = Recorder(args, dead)
                with torch.no_grad():
                    res = getattr(m, w)(**args)
                res = res if isinstance(res, tuple) else () if res is None else (res,)
                got.append((rec.calls, [(tuple(t.shape), str(t.dtype), t.is_contiguous()) for t in res]))
            (old_calls, old_res), (new_calls, new_res) = got
            if old_calls[:2] == [new_calls[0]] * 2 and new_calls[0][0] == "fa_forward_paged_wide_plan" and old_calls[1:] == new_calls:
                wide.append(rid)  # the expected difference: PARENT's second, identical request for the wide plan
            elif old_calls != new_calls:
                diffs.append((w, rid, old_calls, new_calls))
            if old_res != new_res:
                diffs.append((w, rid, old_res, new_res))
    finally:
        torch.cuda.device, _lib._tls.override = real[0], None
        for m, saved in zip(mods, real[1:]):
            m._check_device_tensors, m._stream_handle = saved
    return todo, diffs, wide


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    old = load(parent_text(args[0]), "_parent_flash_attention")
    table, diffs = part1((old, NEW))
    print("Part 1 (exception type and whole text): cases compared per wrapper")
    for w in WRAPPERS:
        print(f"  {w}: {sum(r[0] == w for r in table[0])}")
    kinds = sorted({r[2] for r in table[0]})
    print(f"  {len(table[0])} cases ({', '.join(f'{sum(r[2] == k for r in table[0])} {k}' for k in kinds)}), "
          f"{len(diffs)} differences")
    for a, b in diffs[:20]:
        print("   ", a, "!=", b)
    bad = [r for r in table[0] if r[1].startswith("valid") and "there is no CPU kernel" not in r[3]]
    print(f"  valid calls that do not end in the no-CPU-kernel error: {len(bad)}")
    todo, diffs2, wide = part2((old, NEW))
    print("Part 2 (calls that reach the library, and what returns): routes compared per wrapper")
    for w in WRAPPERS:
        if any(r[0] == w for r in todo):
            print(f"  {w}: {sum(r[0] == w for r in todo)}")
    print(f"  {len(todo)} routes, {len(diffs2)} differences beside the expected one")
    print(f"  expected difference (one fa_forward_paged_wide_plan call fewer than PARENT) on {len(wide)} routes: "
          f"{', '.join(wide)}; expected on wide, wide_window, wide_tail")
    for d in diffs2[:10]:
        print("   ", *d)
    altered = load(open(NEW.__file__).read().replace("{name} must be an int32 tensor", "{name} has to be an int32 tensor", 1), "_altered")
    check = len(part1((NEW, altered))[1])
    print(f"Self-check: a copy with '{{name}} must be an int32 tensor' altered differs in {check} cases (must be > 0)")
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(e) for e in golden_entries(table[0])) + "\n]\n")
        print(f"wrote {len(table[0])} entries to {os.path.relpath(GOLDEN, ROOT)}")
    sys.exit(1 if diffs or bad or diffs2 or sorted(wide) != ["wide", "wide_tail", "wide_window"] or not check else 0)


if __name__ == "__main__":
    main()
