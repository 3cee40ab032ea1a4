"""CPU tests of the merge entry points (include/fa_api.h, "Merging partial results"): every argument check
of fa_merge_partials / fa_accumulate_parts runs on the host before any device call, and the Python layer
(Part, combined_1d / combined_2d, merge_partials) validates before any device work.  No device compute."""

import ctypes

import pytest
import torch

from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

INVALID = _lib.FA_ERR_INVALID_ARGUMENT


def _arr(vals):
    return None if vals is None else _lib.pointer_array(vals)


# distinct non-null addresses: the checks under test return before anything dereferences them
IN = [0x1000 * (i + 1) for i in range(3 * 9)]
O_IN, L_IN, M_IN = IN[0:9], IN[9:18], IN[18:27]
O_OUT, L_OUT, M_OUT = 0x100000, 0x200000, 0x300000


def _merge(dtype=_lib.F16, b=2, nq=16, v_d=8, n=2, Os=O_IN, ls=L_IN, ms=M_IN, O=O_OUT, l=L_OUT, m=M_OUT):
    cut = lambda xs: None if xs is None else xs[:max(n, 1)]  # noqa: E731
    return _lib.lib().fa_merge_partials(None, dtype, b, nq, v_d, n, _arr(cut(Os)), _arr(cut(ls)), _arr(cut(ms)),
                                        O, l, m)


def _accumulate(dtype=_lib.F32, count=64, n=2, parts=O_IN, out=O_OUT):
    return _lib.lib().fa_accumulate_parts(None, dtype, count, n,
                                          _arr(None if parts is None else parts[:max(n, 1)]), out)


MERGE_INVALID = {
    "dtype_low": dict(dtype=-1),
    "dtype_high": dict(dtype=3),
    "no_parts": dict(n=0),
    "nine_parts": dict(n=9),
    "negative_parts": dict(n=-1),
    "negative_b": dict(b=-1),
    "negative_nq": dict(nq=-1),
    "negative_v_d": dict(v_d=-1),
    "zero_v_d": dict(v_d=0),
    "null_O_array": dict(Os=None),
    "null_l_array": dict(ls=None),
    "null_m_array": dict(ms=None),
    "null_O_part": dict(Os=[O_IN[0], 0]),
    "null_l_part": dict(ls=[0, L_IN[1]]),
    "null_m_part": dict(ms=[M_IN[0], 0]),
    "null_O": dict(O=None),
    "null_l": dict(l=None),
    "null_m": dict(m=None),
    "O_aliases_O_part": dict(O=O_IN[1]),
    "l_aliases_l_part": dict(l=L_IN[0]),
    "m_aliases_m_part": dict(m=M_IN[1]),
    "O_aliases_m_part": dict(O=M_IN[0]),
}


@pytest.mark.parametrize("case", sorted(MERGE_INVALID))
def test_merge_rejects(case):
    assert _merge(**MERGE_INVALID[case]) == INVALID
    assert _lib.last_error() != ""
    assert _lib.lib().fa_error_string(INVALID) == b"invalid argument"


def test_merge_messages_name_the_fault():
    _merge(dtype=7)
    assert "dtype" in _lib.last_error()
    _merge(n=9)
    assert "n_parts" in _lib.last_error() and "8" in _lib.last_error()
    _merge(O=O_IN[1])
    assert "aliases" in _lib.last_error() and "part 1" in _lib.last_error()
    _merge(ls=[L_IN[0], 0])
    assert "null" in _lib.last_error() and "part 1" in _lib.last_error()


@pytest.mark.parametrize("kw", [dict(b=0), dict(nq=0), dict(b=0, nq=0),
                                # nothing to do: the pointers are not looked at
                                dict(b=0, Os=None, ls=None, ms=None, O=None, l=None, m=None)])
def test_merge_zero_size_is_ok(kw):
    assert _merge(**kw) == _lib.FA_OK


def test_merge_bad_arguments_win_over_zero_size():
    assert _merge(b=0, dtype=5) == INVALID
    assert _merge(nq=0, n=0) == INVALID
    assert _merge(b=0, nq=-3) == INVALID


ACC_INVALID = {
    "dtype_low": dict(dtype=-1),
    "dtype_high": dict(dtype=3),
    "no_parts": dict(n=0),
    "nine_parts": dict(n=9),
    "negative_count": dict(count=-1),
    "null_array": dict(parts=None),
    "null_part": dict(parts=[O_IN[0], 0]),
    "null_out": dict(out=None),
    "out_aliases_part": dict(out=O_IN[1]),
}


@pytest.mark.parametrize("case", sorted(ACC_INVALID))
def test_accumulate_rejects(case):
    assert _accumulate(**ACC_INVALID[case]) == INVALID
    assert _lib.last_error() != ""


def test_accumulate_zero_size_is_ok():
    assert _accumulate(count=0) == _lib.FA_OK
    assert _accumulate(count=0, parts=None, out=None) == _lib.FA_OK
    assert _accumulate(count=0, n=9) == INVALID


def test_max_parts_agrees_with_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fa_api.h")).read()
    assert int(re.search(r"#define FA_MAX_PARTS (\d+)", header).group(1)) == _lib.FA_MAX_PARTS == fa.MAX_PARTS == 8


# ------------------------------------------------------------------ Python validation, on CPU tensors
def _t(*shape, dt=torch.float16):
    return torch.zeros(shape, dtype=dt)


def test_combined_is_exported():
    import tf_flash_attention_amd as pkg
    for name in ("Part", "combined_1d", "combined_2d", "merge_partials"):
        assert name in fa.__all__ and getattr(pkg, name) is getattr(fa, name)
    assert len(vars(fa._fa_kernel)) == 30


def test_combined_rejects_mismatched_batch_shape():
    Q = _t(2, 3, 8, 16)
    good = fa.Part("full", _t(2, 3, 8, 4), _t(2, 3, 8, 4))
    bad = fa.Part("local", _t(2, 4, 8, 16), _t(2, 4, 8, 16), window_size=3)
    with pytest.raises(fa.InvalidArgumentError, match=r"The batch shape of all inputs should be equal, but "
                                                      r"Q_batch_shape = \[2,3\], K_batch_shape = \[2,4\]"):
        fa.combined_1d(Q, [good, bad])


def test_combined_rejects_mismatched_channels():
    Q = _t(2, 8, 16)
    with pytest.raises(fa.InvalidArgumentError, match="The channel dimension of Q and K should be equal"):
        fa.combined_1d(Q, [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4)), fa.Part("causal", _t(2, 6, 16), _t(2, 8, 16))])
    with pytest.raises(fa.InvalidArgumentError, match="The sequence shape of K and V are expected to be equal"):
        fa.combined_2d(_t(2, 8, 4, 4), [fa.Part("full", _t(2, 8, 2, 4), _t(2, 8, 4, 2))])


def test_combined_rejects_mismatched_v_channels_across_parts():
    Q = _t(2, 8, 16)
    with pytest.raises(fa.InvalidArgumentError, match="The channel dimension of V should be equal in all parts, "
                                                      "but 8 and 12 were received"):
        fa.combined_1d(Q, [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4)), fa.Part("full", _t(2, 8, 5), _t(2, 12, 5))])


def test_combined_rejects_mixed_dtypes():
    Q = _t(2, 8, 16)
    with pytest.raises(TypeError, match="share one dtype"):
        fa.combined_1d(Q, [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4)),
                           fa.Part("full", _t(2, 8, 4, dt=torch.float32), _t(2, 8, 4, dt=torch.float32))])
    with pytest.raises(TypeError, match="unsupported dtype"):
        fa.combined_1d(_t(2, 8, 16, dt=torch.bfloat16), [fa.Part("full", _t(2, 8, 4, dt=torch.bfloat16),
                                                                 _t(2, 8, 4, dt=torch.bfloat16))])


@pytest.mark.parametrize("n", [0, 9])
def test_combined_rejects_part_counts(n):
    Q = _t(2, 8, 16)
    with pytest.raises(fa.InvalidArgumentError, match=rf"The number of parts should be in \[1, 8\], but {n} were"):
        fa.combined_1d(Q, [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4)) for _ in range(n)])
    with pytest.raises(fa.InvalidArgumentError, match=r"The number of parts should be in \[1, 8\]"):
        fa.merge_partials([_t(2, 8, 16)] * n, [_t(2, 16, dt=torch.float32)] * n, [_t(2, 16)] * n)


def test_part_and_sync_mode_are_checked():
    with pytest.raises(fa.InvalidArgumentError, match="Unsupported policy: banded"):
        fa.Part("banded", _t(2, 8, 4), _t(2, 8, 4))
    with pytest.raises(fa.InvalidArgumentError, match="Unsupported sync_mode: middle"):
        fa.combined_1d(_t(2, 8, 16), [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4), sync_mode="middle")])
    with pytest.raises(TypeError, match="Part records"):
        fa.combined_1d(_t(2, 8, 16), [(_t(2, 8, 4), _t(2, 8, 4))])


def test_cpu_tensors_fail_loudly_after_validation():
    """Well-formed CPU inputs reach the device check: there is no CPU kernel and no eager fallback."""
    with pytest.raises(fa.InvalidArgumentError, match="ROCm"):
        fa.combined_1d(_t(2, 8, 16), [fa.Part("full", _t(2, 8, 4), _t(2, 8, 4))])
    with pytest.raises(fa.InvalidArgumentError, match="ROCm"):
        fa.merge_partials([_t(2, 8, 16)], [_t(2, 16, dt=torch.float32)], [_t(2, 16)])


def test_merge_partials_validates_shapes_and_dtypes():
    O, l, m = _t(2, 8, 16), _t(2, 16, dt=torch.float32), _t(2, 16)
    with pytest.raises(fa.InvalidArgumentError, match="numbers of O, l and m partials"):
        fa.merge_partials([O, O], [l], [m, m])
    with pytest.raises(fa.InvalidArgumentError, match=r"shapes of all O partials should be equal, but \[2,8,16\] and "
                                                      r"\[2,8,12\]"):
        fa.merge_partials([O, _t(2, 8, 12)], [l, l], [m, m])
    with pytest.raises(fa.InvalidArgumentError, match="without its channel dimension"):
        fa.merge_partials([O], [_t(2, 8, dt=torch.float32)], [m])
    with pytest.raises(TypeError, match="l must be torch.float32"):
        fa.merge_partials([O], [l.half()], [m])
    with pytest.raises(TypeError, match="must have dtype torch.float16"):
        fa.merge_partials([O], [l], [m.float()])
    # 2d: the channel axis is found from seq_dims
    with pytest.raises(fa.InvalidArgumentError, match="ROCm"):
        fa.merge_partials([_t(2, 8, 4, 4)], [_t(2, 4, 4, dt=torch.float32)], [_t(2, 4, 4)], seq_dims=2)


def test_pointer_array_layout():
    arr = _lib.pointer_array([0x10, 0, 0x30])
    assert ctypes.sizeof(arr) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [arr[i] for i in range(3)] == [0x10, None, 0x30]
    assert _lib.pointer_array(None) is None
