"""OCP FP8 e4m3fn in numpy: the decode table of all 256 bytes and a round-to-nearest-even saturating encoder
(DESIGN.md §3.11).  The only source of quantized test data and of the dequantized float64 reference of the FP8
K/V cache tests; tests/test_fp8_ref.py checks both against torch.float8_e4m3fn on the CPU.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 (0x7F, 0xFF) is NaN, so the largest
finite value is S.1111.110 = 448; exponent 0 is subnormal, m / 8 * 2^-6."""

import numpy as np

MAX = 448.0


def _decode_table():
    b = np.arange(256)
    s, e, m = b >> 7, (b >> 3) & 15, (b & 7).astype(np.float64)
    v = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(s == 1, -v, v)


TABLE = _decode_table()      # float64 value of every byte (exact)
_FINITE = TABLE[:127]        # bytes 0x00 .. 0x7E: the non-negative finite values, ascending


def decode(b8):
    """uint8 array -> float64 array of the same shape (exact; NaN for 0x7F / 0xFF)."""
    return TABLE[np.asarray(b8, dtype=np.uint8)]


def encode(x):
    """float array -> uint8 array: round to nearest, ties to the even code, saturating at +-448 (no NaN from a
    finite input, unlike a plain cast); NaN -> 0x7F with the sign bit kept."""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(np.where(np.isnan(x), 0.0, x)), MAX)
    hi = np.clip(np.searchsorted(_FINITE, a, side="left"), 1, 126)  # _FINITE[hi - 1] <= a <= _FINITE[hi] (a > 0)
    lo = hi - 1
    dl, dh = a - _FINITE[lo], _FINITE[hi] - a                       # exact: neighbours within a factor of two
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(x), 0x7F, code)
    return (code | (np.signbit(x).astype(np.int64) << 7)).astype(np.uint8)


def quantize(x, scale, head_axis):
    """x / scale[h] along head_axis, encoded: the bytes whose true values are scale[h] * decode(bytes)."""
    shape = [1] * np.ndim(x)
    shape[head_axis] = -1
    return encode(np.asarray(x, dtype=np.float64) / np.asarray(scale, dtype=np.float64).reshape(shape))


def dequantize(b8, scale, head_axis):
    """float64 scale[h] * decode(bytes) with the scale as the float32 value the kernels read."""
    shape = [1] * np.ndim(b8)
    shape[head_axis] = -1
    return decode(b8) * np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(shape)
