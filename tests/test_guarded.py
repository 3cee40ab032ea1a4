"""The guarded checker (tests/guarded.py) rejects what it is meant to reject: on the CPU, with numpy stand-ins for the
kernels, through the assertion code tests/test_gpu_guarded.py runs on the GPU (as tests/test_gate_mutations.py shows
it for the gradient gate).

The correct stand-in is the float64 oracle rounded to the tensor type; each wrong one is that plus one planted defect:

  past_O       writes one element past the end of O
  before_dK    writes one element before dK
  skip_dQ      leaves one element of dQ unwritten
  v_tail       adds 0 * (the element after V's last) to O
  ws_read      starts a dQ sum from a workspace word it never wrote
  alter_input  writes an element of K

Each must fail with the right tensor named in the message.  Also here: the geometry of a Guarded tensor."""
import numpy as np
import pytest
import torch

from oracle import fa_oracle as O
from tests import guarded
from tests.guarded import GUARD, Guarded
from tests.test_gpu_parity import check_outputs, oracle_outputs

CPU = torch.device("cpu")
DT = np.float16
B, D, VD, NQ, NK = 3, 8, 6, 5, 7          # odd lengths: no tensor's size is a multiple of 16 bytes
PROB = O.Problem("causal", 1, "scale_end")
DEFECTS = {  # defect -> (the tensor the message must name, a phrase of the assertion that must fire)
    "past_O": ("O", "outside the tensor"),
    "before_dK": ("dK", "outside the tensor"),
    "skip_dQ": ("dQ", "run A != run B"),
    "v_tail": ("O", "run A != run B"),
    "ws_read": ("dQ", "run A != run B"),
    "alter_input": ("K", "the input was written"),
}


def _inputs():
    rng = np.random.default_rng(5)
    return {n: rng.uniform(-2, 2, s).astype(DT)
            for n, s in (("Q", (B, D, NQ)), ("K", (B, D, NK)), ("V", (B, VD, NK)), ("dO", (B, VD, NQ)))}


def _body(g):
    return g.t.numpy()                    # shares the Guarded's memory on the CPU


def _elem(g, index):
    """A one-element view at `index` elements from the body's first (-1: just before it; g.t.numel(): just past it)."""
    isz = g.dtype.itemsize
    at = g.front + index * isz
    return g.raw.numpy()[at:at + isz].view(g.dtype)


def _forward(defect):
    def call(bufs, ws):
        o, l, m = O.forward(_body(bufs["Q"]), _body(bufs["K"]), _body(bufs["V"]), PROB)
        if defect == "v_tail":
            with np.errstate(invalid="ignore"):
                o = (o.astype(np.float64) + 0.0 * float(_elem(bufs["V"], bufs["V"].t.numel())[0])).astype(DT)
        _body(bufs["O"])[...], _body(bufs["l"])[...], _body(bufs["m"])[...] = o, l, m
        if defect == "past_O":
            _elem(bufs["O"], bufs["O"].t.numel())[0] = 1.0
        if defect == "alter_input":
            _body(bufs["K"])[1, 2, 3] = 0.5
        return 0
    return call


def _backward(defect):
    def call(bufs, ws):
        dq, dk, dv = (x.astype(DT) for x in O.backward_f64(*(_body(bufs[n]) for n in ("Q", "K", "V", "dO")), PROB))
        if defect == "ws_read":            # a partial sum that starts from the scratch word instead of from zero
            acc = ws.raw.numpy()[ws.front:ws.front + 4].view(np.float32)
            with np.errstate(over="ignore"):
                acc[0] += np.float32(dq[1, 2, 3])
                dq[1, 2, 3] = DT(acc[0])
        if defect == "skip_dQ":
            keep = _body(bufs["dQ"])[2, 7, 4].copy()
        _body(bufs["dQ"])[...], _body(bufs["dK"])[...], _body(bufs["dV"])[...] = dq, dk, dv
        if defect == "skip_dQ":
            _body(bufs["dQ"])[2, 7, 4] = keep
        if defect == "before_dK":
            _elem(bufs["dK"], -1)[0] = 1.0
        return 0
    return call


def _run(defect, variants=None):
    x = _inputs()
    specs = {"O": ((B, VD, NQ), DT), "l": ((B, NQ), np.float32), "m": ((B, NQ), DT),
             "dQ": ((B, D, NQ), DT), "dK": ((B, D, NK), DT), "dV": ((B, VD, NK), DT)}
    args = (DT, PROB.policy, 1, PROB.sync_mode, D, VD, (NQ,), (NK,), 1, 0, False, x["Q"], x["K"], x["V"], x["dO"])
    oracle = oracle_outputs(DT, PROB.policy, 1, PROB.sync_mode, 1, 0, False, x["Q"], x["K"], x["V"], x["dO"],
                            list(range(B)), True)
    seen = []

    def check(variant, res):
        seen.append(variant)
        check_outputs(*args, res["O"], res["l"], res["m"], (res["dQ"], res["dK"], res["dV"]), oracle=oracle)

    guarded.guarded_case("stand-in", x, specs, CPU, _forward(defect), _backward(defect), 0, 256, check, variants)
    return seen


def test_the_correct_stand_in_passes_under_every_variant():
    assert tuple(_run(None)) == guarded.BWD_VARIANTS


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("variant", ["none", "all"])
def test_a_wrong_stand_in_is_rejected_with_its_tensor_named(defect, variant):
    tensor, phrase = DEFECTS[defect]
    with pytest.raises(AssertionError) as e:
        _run(defect, [variant])
    msg = str(e.value)
    assert f"[{variant}]" in msg and f": {tensor}: " in msg and phrase in msg and "stand-in" in msg, msg


def test_the_oracle_gate_is_part_of_the_check():
    """Assertion 5: a stand-in that is in bounds, deterministic and wrong (O scaled by 1.01) passes 1-4 and fails the
    gate."""
    def forward(bufs, ws):
        _forward(None)(bufs, ws)
        _body(bufs["O"])[...] = (_body(bufs["O"]).astype(np.float64) * 1.01).astype(DT)
        return 0
    x = _inputs()
    specs = {"O": ((B, VD, NQ), DT), "l": ((B, NQ), np.float32), "m": ((B, NQ), DT)}

    def check(variant, res):
        check_outputs(DT, PROB.policy, 1, PROB.sync_mode, D, VD, (NQ,), (NK,), 1, 0, False, x["Q"], x["K"], x["V"],
                      x["dO"], res["O"], res["l"], res["m"])

    with pytest.raises(AssertionError, match="O: .* elements off"):
        guarded.guarded_case("stand-in", x, specs, CPU, forward, check=check, variants=["none"])


def test_a_failed_status_is_reported():
    x = _inputs()
    specs = {"O": ((B, VD, NQ), DT), "l": ((B, NQ), np.float32), "m": ((B, NQ), DT)}
    with pytest.raises(AssertionError, match=r"stand-in forward \[Q\] run A: status -2"):
        guarded.guarded_case("stand-in", x, specs, CPU, lambda bufs, ws: -2, variants=["Q"])


# ------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_placement(dtype, offset):
    isz = np.dtype(dtype).itemsize
    g = Guarded((3, 5), dtype, CPU, offset, 0xFF, 0xA5)
    assert g.raw.data_ptr() % 256 == 0
    assert g.data_ptr() == g.raw.data_ptr() + GUARD + offset * isz
    assert (g.data_ptr() % 16 == 0) == (offset == 0) and g.data_ptr() % isz == 0
    assert g.raw.numel() == GUARD + offset * isz + 15 * isz + GUARD and g.nbytes == 15 * isz
    raw = g.raw.numpy()
    assert (raw[:g.front] == 0xFF).all() and (raw[g.front + g.nbytes:] == 0xFF).all()
    assert (raw[g.front:g.front + g.nbytes] == 0xA5).all() and g.body_bytes() == b"\xa5" * g.nbytes
    assert g.intact() and g.stray().size == 0
    # every guard byte is watched, the nearest and the farthest ones included; the body is not
    for at in (0, g.front - 1, g.front + g.nbytes, raw.size - 1):
        raw[at] ^= 1
        assert not g.intact() and g.stray().tolist() == [at - g.front]
        raw[at] ^= 1
    raw[g.front] ^= 1
    raw[g.front + g.nbytes - 1] ^= 1
    assert g.intact()


def test_the_rear_guard_starts_inside_the_last_16_byte_chunk_of_an_odd_sized_tensor():
    g = Guarded((3, 5), np.float16, CPU, 0, 0x00)       # 30 bytes from a 16-byte boundary
    end = g.data_ptr() + g.nbytes
    assert g.data_ptr() % 16 == 0 and end % 16 == 14
    g.upload(np.ones((3, 5), np.float16))
    # a 16-byte store of the last chunk's 7 elements would also write the 2 bytes at offsets 30, 31
    g.raw.numpy()[g.front + 16:g.front + 32] = 0x3C
    assert g.stray().tolist() == [30, 31]


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_input_guards_decode_to_nan(dtype):
    g = Guarded((7,), dtype, CPU, 1, guarded.IN_FILLS[0]).upload(np.arange(7).astype(dtype))
    isz = np.dtype(dtype).itemsize
    before = g.raw.numpy()[g.front - 4 * isz:g.front].view(dtype)
    after = g.raw.numpy()[g.front + g.nbytes:g.front + g.nbytes + 4 * isz].view(dtype)
    assert np.isnan(before).all() and np.isnan(after).all()
    assert np.array_equal(g.numpy(), np.arange(7).astype(dtype)) and g.intact()
    zero = Guarded((7,), dtype, CPU, 0, guarded.IN_FILLS[1])
    assert (zero.raw.numpy()[:zero.front].view(dtype) == 0).all()


def test_fills_differ_in_every_byte_and_variants_name_their_tensors():
    assert guarded.OUT_FILLS[0] ^ guarded.OUT_FILLS[1] == 0xFF and set(guarded.IN_FILLS) == {0xFF, 0x00}
    assert guarded.variant_offsets("none", guarded.BWD_TENSORS) == dict.fromkeys(guarded.BWD_TENSORS, 0)
    assert guarded.variant_offsets("all", guarded.FWD_TENSORS) == dict.fromkeys(guarded.FWD_TENSORS, 1)
    assert guarded.variant_offsets("dK", guarded.BWD_TENSORS) == {**dict.fromkeys(guarded.BWD_TENSORS, 0), "dK": 1}
