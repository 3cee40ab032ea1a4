"""What the decode-family wrappers raise, whole: exception type, full text and, through the cases with two faults, which
check comes first.  ``tests/golden/wrapper_messages.json`` was recorded by ``tools/wrapper_parity.py PARENT --record``
from the module as it stood before its checks were folded into shared helpers; the cases are that tool's own (no second
copy here).  The other ``test_*_api.py`` files match fragments of these messages; this one keeps a copied check from
drifting in wording or order.  CPU only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wrapper_parity  # noqa: E402
from tf_flash_attention_amd import flash_attention as fa  # noqa: E402

GOLDEN = wrapper_parity.load_golden()
CASES = wrapper_parity.cases()


def test_the_golden_holds_the_tools_cases():
    ids = [(w, cid) for w, cid, _ in CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == set(GOLDEN)
    assert {w for w, _ in ids} == set(wrapper_parity.WRAPPERS)


@pytest.mark.parametrize("wrapper", wrapper_parity.WRAPPERS)
def test_every_case_raises_the_recorded_type_and_text(wrapper):
    wrong = []
    for w, cid, run in CASES:
        if w == wrapper:
            got = wrapper_parity.outcome(fa, w, run)
            if got != GOLDEN[(w, cid)]:
                wrong.append((cid, got, GOLDEN[(w, cid)]))
    assert not wrong, f"{len(wrong)} cases of {wrapper} differ from the golden, the first: {wrong[0]}"


@pytest.mark.parametrize("wrapper", wrapper_parity.WRAPPERS)
def test_the_valid_call_reaches_the_device_check(wrapper):
    run = next(run for w, cid, run in CASES if (w, cid) == (wrapper, "valid"))
    assert wrapper_parity.outcome(fa, wrapper, run) == (
        "InvalidArgumentError", "flash attention tensors must live on a ROCm (cuda) device; there is no CPU kernel")
