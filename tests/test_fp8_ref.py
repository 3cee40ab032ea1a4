"""tests/fp8_ref.py against torch.float8_e4m3fn on the CPU: the decode of every byte and the encoder on a seeded
sweep inside +-448, on every representable value, on every midpoint between neighbours (the ties) and on the
saturating side, where the two differ on purpose."""

import numpy as np
import torch

from tests import fp8_ref

F8 = torch.float8_e4m3fn


def _torch_encode(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(F8).view(torch.uint8).numpy()


def test_decode_of_every_byte():
    ref = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).to(torch.float64).numpy()
    nan = np.isnan(ref)
    assert sorted(np.nonzero(nan)[0].tolist()) == [0x7F, 0xFF]
    assert (np.isnan(fp8_ref.TABLE) == nan).all()
    assert (fp8_ref.TABLE[~nan] == ref[~nan]).all()
    assert (np.signbit(fp8_ref.TABLE[~nan]) == np.signbit(ref[~nan])).all()
    assert fp8_ref.TABLE[0x7E] == fp8_ref.MAX and fp8_ref.TABLE[0x01] == 2.0 ** -9
    # every value is an fp16 value: the forward's conversion of the cache to fp16 loses nothing
    assert (fp8_ref.TABLE[~nan].astype(np.float16).astype(np.float64) == fp8_ref.TABLE[~nan]).all()


def test_encode_round_trips_every_finite_byte():
    b = np.array([i for i in range(256) if i not in (0x7F, 0xFF)], dtype=np.uint8)
    assert (fp8_ref.encode(fp8_ref.decode(b)) == b).all()


def test_encode_on_a_seeded_sweep_inside_the_range():
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.uniform(-448, 448, 20000), rng.uniform(-2, 2, 20000), rng.uniform(-2.0 ** -5, 2.0 ** -5, 20000),
                        rng.standard_normal(20000) * np.exp2(rng.integers(-12, 9, 20000))]).astype(np.float32)
    x = x[np.abs(x) <= 448]
    assert (fp8_ref.encode(x) == _torch_encode(x)).all()


def test_encode_ties_go_to_the_even_code():
    v = fp8_ref.TABLE[:127]
    mid = (v[:-1] + v[1:]) / 2  # exact in float32: one more mantissa bit
    for sign in (1.0, -1.0):
        x = (sign * mid).astype(np.float32)
        got = fp8_ref.encode(x)
        assert (got == _torch_encode(x)).all()
        assert ((got & 1) == 0).all()
    assert fp8_ref.encode(np.array([0.0, -0.0])).tolist() == [0x00, 0x80]
    assert (fp8_ref.encode(np.array([-0.0, -1e-9], np.float32)) == _torch_encode(np.array([-0.0, -1e-9]))).all()


def test_encode_saturates_where_the_plain_cast_does_not():
    x = np.array([448.0, 464.0, 465.0, 500.0, 1e9, -500.0, np.inf, -np.inf])
    assert fp8_ref.encode(x).tolist() == [0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x7E, 0xFE]
    assert np.isnan(torch.tensor([500.0]).to(F8).float().numpy()).all()  # why quantize_kv_fp8 clamps before its cast
    assert fp8_ref.encode(np.array([np.nan])).tolist()[0] & 0x7F == 0x7F


def test_quantize_and_dequantize_per_head():
    rng = np.random.default_rng(9)
    x = rng.uniform(-2, 2, (3, 2, 5, 7))
    scale = np.array([0.037, 300.0], np.float32)
    b8 = fp8_ref.quantize(x, scale, 1)
    back = fp8_ref.dequantize(b8, scale, 1)
    assert b8.dtype == np.uint8 and back.shape == x.shape
    # within half a step of the grid: 2^-4 relative for normals, half the subnormal step 2^-10 otherwise
    s = scale.astype(np.float64).reshape(1, 2, 1, 1)
    assert (np.abs(back - x) <= np.maximum(np.abs(x) * 2.0 ** -4, s * 2.0 ** -10) + 1e-12).all()
