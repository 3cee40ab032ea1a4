"""CPU test of tools/prefill_time.py's plumbing: the grid it times, the statistics and the
criterion it derives from the windows' times, its argument checks, and that it refuses to run without a GPU."""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prefill_time as T  # noqa: E402


def test_the_grid_is_the_issues_without_the_delegated_combinations():
    grid = T.shapes()
    main = [(s["g"], s["nq"], s["d"]) for s in grid if not s.get("control")]
    want = [(g, nq, d) for d in (64, 128) for g in (1, 4, 8) for nq in (32, 128, 512) if g * nq > 128]
    assert main == want and len(main) == 12
    assert all(s["seqs"] == 16 and s["hk"] == 2 for s in grid if not s.get("control"))
    control = [s for s in grid if s.get("control")]
    assert [(s["seqs"] * s["hk"], s["nq"], s["d"]) for s in control] == [(1024, 128, 64), (1024, 128, 128)]
    for s in grid:
        for page in T.PAGES:
            chunks, chunk, pb, rows, nqb, delegated = T.prefill_plan(s["g"], s["nq"], T.CAP, s["d"], page)
            assert not delegated and nqb >= 2 and s["nq"] % pb == 0 and chunks * chunk >= T.CAP


def test_statistics_and_criterion():
    times = dict(prefill=[1.0, 1.1, 0.9, 1.0, 1.0, 1.0, 1.0], loop=[2.0, 2.0, 2.0, 2.2, 2.0, 2.0, 2.0],
                 loop_copy=[3.0] * 7)
    s = T.summarise(times)
    assert s["prefill_ms"] == dict(median=1.0, min=0.9, max=1.1, spread=pytest.approx(0.2))
    assert s["loop_ms"]["spread"] == pytest.approx(0.1) and s["loop_copy_ms"]["spread"] == 0.0
    assert s["loop_over_prefill"] == 2.0 and s["loop_copy_over_prefill"] == 3.0
    assert s["twice_the_larger_spread"] == pytest.approx(0.4) and s["prefill_beats_loop"] is True
    # a gain inside twice the larger spread does not count, nor does a loss
    assert T.summarise(dict(times, loop=[1.3] * 7))["prefill_beats_loop"] is False
    assert T.summarise(dict(times, loop=[0.5] * 7))["prefill_beats_loop"] is False


def test_arguments_and_no_gpu():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prefill_time.py"), *a],  # noqa: E731
                                    capture_output=True, text=True, timeout=120)
    r = run("--repeats", "3")
    assert r.returncode == 2 and "at least 5" in r.stderr
    if not torch.cuda.is_available():
        r = run()
        assert r.returncode != 0 and "no GPU" in r.stderr
