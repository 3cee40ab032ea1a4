"""Guard bands and mixed alignments for the dense entry points (no GPU at import; works on any torch device).

A `Guarded` tensor lives inside one uint8 allocation, between two guard bands of GUARD bytes, at a chosen element
offset from a 256-byte aligned base.  `guarded_pair` runs one call twice over such tensors,

    run A: input guards 0xFF (NaN in fp16, fp32 and fp64), outputs and workspace (bodies AND guards) 0xA5
    run B: input guards 0x00,                              outputs and workspace (bodies AND guards) 0x5A

and asserts, in this order and each with a message that names the case, the variant, the tensor and the first
offending byte offsets:

  1. both calls return status 0;
  2. every guard byte of every tensor, the workspace included, is what it was filled with (a store outside a tensor);
  3. every input's body is byte for byte what was uploaded (a store into an input);
  4. every output of run A is bitwise run B's.  An element no lane wrote differs (0xA5 against 0x5A); a result that
     depends on bytes outside an input, or on what the workspace held before the call, differs (NaN or 0xFF against
     zero or 0x5A).

`guarded_case` runs a forward and a backward that way for each alignment variant (the named tensors one element off
a 16-byte boundary, the others on a 256-byte one; the workspace always on one: it is the library's own layout) and
hands run A's results to the caller's oracle check.  The `forward` / `backward` callables are the kernels under
test: the C ABI on the GPU (tests/test_gpu_guarded.py), numpy stand-ins with planted defects on the CPU
(tests/test_guarded.py), through the same assertion code.

What this cannot see: an access farther than GUARD = 4096 bytes from the tensor it belongs to (it lands in another
allocation or in allocator slack), and a read outside a tensor that happens not to change a result for either
fill.
"""

import numpy as np
import torch

# Not a measurement but a condition: wider, by a wide margin, than the widest access (16 bytes) plus any align-down
# of its address; and a multiple of 256, so that offset_elems = 0 keeps the body on a 256-byte boundary.
GUARD = 4096
IN_FILLS = (0xFF, 0x00)    # run A, run B: the guards of an input
OUT_FILLS = (0xA5, 0x5A)   # run A, run B: the guards and the body of an output or a workspace
FWD_TENSORS = ("Q", "K", "V", "O", "l", "m")
BWD_TENSORS = ("Q", "K", "V", "O", "l", "m", "dO", "dQ", "dK", "dV")
FWD_VARIANTS = ("none", "all") + FWD_TENSORS
BWD_VARIANTS = ("none", "all") + BWD_TENSORS

_TORCH = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32,
          np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}


class Guarded:
    """A contiguous tensor of `shape` and numpy `dtype` on `device` with GUARD bytes of `guard_fill` before its first
    and after its last element.

    One uint8 allocation holds GUARD + offset_elems * itemsize + nbytes + GUARD bytes (`.raw`); `.t` views the body at
    base + GUARD + offset_elems * itemsize.  The base is 256-byte aligned (the allocation is cut to that), so the
    body is 256-byte aligned for offset_elems = 0 and off every 16-byte boundary for an offset that is no multiple
    of 16 bytes: data_ptr() % 16 == 0 exactly when offset_elems == 0 is asserted.  The rear guard begins at the byte
    after the last element, with no rounding: a tensor whose size is not a multiple of 16 bytes has guard bytes
    inside its last 16-byte chunk.  body_fill (a byte) fills the body too; None leaves it for upload().

    A stray access farther than GUARD = 4096 bytes from the body is out of sight."""

    def __init__(self, shape, dtype, device, offset_elems=0, guard_fill=0xA5, body_fill=None):
        self.shape = tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        self.guard_fill = int(guard_fill)
        self.offset_elems = int(offset_elems)
        assert 0 <= self.offset_elems * self.dtype.itemsize < 256 and GUARD % 256 == 0 and GUARD >= 16 * 16
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.front = GUARD + self.offset_elems * self.dtype.itemsize          # bytes before the body
        total = self.front + self.nbytes + GUARD
        # (the GPU's caching allocator hands out 512-byte aligned blocks: pad is 0 there; the CPU's only 64-byte ones)
        store = torch.empty(total + 255, dtype=torch.uint8, device=device)
        pad = -store.data_ptr() % 256
        self.raw = store[pad:pad + total]
        assert self.raw.data_ptr() % 256 == 0 and self.raw.numel() == total
        self.raw.fill_(self.guard_fill)
        body = self.raw[self.front:self.front + self.nbytes]
        if body_fill is not None:
            body.fill_(int(body_fill))
        self.t = body.view(_TORCH[self.dtype]).view(self.shape)
        assert self.t.is_contiguous() and self.t.data_ptr() == self.raw.data_ptr() + self.front
        assert (self.t.data_ptr() % 16 == 0) == (self.offset_elems == 0), (self.t.data_ptr(), self.offset_elems)
        assert self.t.data_ptr() % self.dtype.itemsize == 0

    def upload(self, x):
        x = np.ascontiguousarray(x)
        assert x.dtype == self.dtype and x.shape == self.shape, (x.dtype, x.shape, self.dtype, self.shape)
        self.t.copy_(torch.from_numpy(x))
        return self

    def data_ptr(self):
        return self.t.data_ptr()

    def _bytes(self):
        return self.raw.cpu().numpy()

    def stray(self):
        """Byte offsets, relative to the body's first byte, of every guard byte that is no longer guard_fill:
        negative in the front guard, >= nbytes in the rear one."""
        raw = self._bytes()
        bad = np.nonzero(raw != self.guard_fill)[0].astype(np.int64) - self.front
        return bad[(bad < 0) | (bad >= self.nbytes)]

    def intact(self):
        return self.stray().size == 0

    def body_bytes(self):
        return self._bytes()[self.front:self.front + self.nbytes].tobytes()

    def numpy(self):
        """A copy of the body as a numpy array."""
        return np.frombuffer(self.body_bytes(), dtype=self.dtype).reshape(self.shape).copy()


def variant_offsets(variant, names):
    """offset_elems per tensor of `names`: 1 for the tensors the variant names ("all": every one), else 0."""
    assert variant in ("none", "all") or variant in names, (variant, names)
    return {n: int(variant == "all" or variant == n) for n in names}


def _first(offsets, n=4):
    offsets = np.asarray(offsets)
    return f"{offsets[:n].tolist()}{' ...' if offsets.size > n else ''} ({offsets.size} bytes)"


def _diff(a, b):
    return np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]


def guarded_pair(label, variant, inputs, outputs, ws_bytes, offsets, call, device):
    """Runs `call` as run A and as run B and makes assertions 1-4 of the module docstring.

    inputs:  {name: numpy array}, uploaded between guards of IN_FILLS[run];
    outputs: {name: (shape, numpy dtype)}, body and guards filled with OUT_FILLS[run];
    ws_bytes: the workspace, like an output (uint8, never moved off its alignment); 0: no workspace, `call` gets None;
    offsets: {name: offset_elems};  call(bufs: {name: Guarded}, ws: Guarded or None) -> status.
    Returns run A's outputs {name: numpy array}."""
    where = f"{label} [{variant}]"
    runs = []
    for run in (0, 1):
        tag = f"{where} run {'AB'[run]}"
        bufs = {n: Guarded(x.shape, x.dtype, device, offsets.get(n, 0), IN_FILLS[run]).upload(x)
                for n, x in inputs.items()}
        for n, (shape, dt) in outputs.items():
            bufs[n] = Guarded(shape, dt, device, offsets.get(n, 0), OUT_FILLS[run], OUT_FILLS[run])
        ws = Guarded((ws_bytes,), np.uint8, device, 0, OUT_FILLS[run], OUT_FILLS[run]) if ws_bytes else None
        status = call(bufs, ws)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        assert status == 0, f"{tag}: status {status}"
        for n, g in list(bufs.items()) + ([("workspace", ws)] if ws is not None else []):
            bad = g.stray()
            assert bad.size == 0, (f"{tag}: {n}: bytes outside the tensor were written, at byte offsets {_first(bad)} "
                                   f"from its first byte (it holds {g.nbytes} bytes)")
        for n, x in inputs.items():
            bad = _diff(bufs[n].body_bytes(), np.ascontiguousarray(x).tobytes())
            assert bad.size == 0, f"{tag}: {n}: the input was written, at byte offsets {_first(bad)}"
        runs.append({n: bufs[n].body_bytes() for n in outputs})
    for n in outputs:
        bad = _diff(runs[0][n], runs[1][n])
        assert bad.size == 0, (f"{where}: {n}: run A != run B at byte offsets {_first(bad)}: an element nobody wrote, or "
                               f"a result that depends on bytes outside an input or on the workspace's old content")
    return {n: np.frombuffer(runs[0][n], dtype=np.dtype(dt)).reshape(shape).copy()
            for n, (shape, dt) in outputs.items()}


def guarded_case(label, arrays, out_specs, device, forward, backward=None, fwd_ws_bytes=0, bwd_ws_bytes=0, check=None,
                 variants=None):
    """The forward and (with `backward`) the backward of one case under every alignment variant.

    arrays: {"Q", "K", "V", "dO"} numpy inputs; out_specs: {"O", "l", "m", "dQ", "dK", "dV"} -> (shape, dtype).
    forward(bufs, ws) gets the Guarded Q, K, V (inputs) and O, l, m (outputs); backward(bufs, ws) gets Q, K, V, dO and
    run A's own O, l, m of the forward under the same variant as inputs, and dQ, dK, dV as outputs.  A variant that
    names a backward-only tensor (dO, dQ, dK, dV) takes the forward of "none".  check(variant, results) receives run
    A's {"O", "l", "m"[, "dQ", "dK", "dV"]}: assertion 5, the caller's oracle gate."""
    if variants is None:
        variants = BWD_VARIANTS if backward is not None else FWD_VARIANTS
    fwd_done = {}
    for variant in variants:
        fv = variant if variant in FWD_VARIANTS else "none"
        if fv not in fwd_done:
            fwd_done[fv] = guarded_pair(label + " forward", fv, {n: arrays[n] for n in ("Q", "K", "V")},
                                        {n: out_specs[n] for n in ("O", "l", "m")}, fwd_ws_bytes,
                                        variant_offsets(fv, FWD_TENSORS), forward, device)
        res = dict(fwd_done[fv])
        if backward is not None:
            ins = {n: arrays[n] for n in ("Q", "K", "V", "dO")}
            ins.update(res)
            res.update(guarded_pair(label + " backward", variant, ins, {n: out_specs[n] for n in ("dQ", "dK", "dV")},
                                    bwd_ws_bytes, variant_offsets(variant, BWD_TENSORS), backward, device))
        if check is not None:
            check(variant, res)
