"""CPU test of tools/append_time.py's plumbing: the rows it times, the statistics, the criterion and
the rates it derives from the windows' times, its argument checks, and that it refuses to run without a GPU."""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import append_time as T  # noqa: E402


def test_the_rows_are_the_issues():
    grid = T.rows()
    main = [(r["d"], r["page"], r["fp8"], r["n_new"]) for r in grid if not r.get("control")]
    want = [(d, page, fp8, n) for d in (64, 128) for page in (64, 256) for fp8 in (False, True) for n in (1, 128, 2048)]
    assert main == want and len(main) == 24
    assert all(r["seqs"] == 16 and r["hk"] == 2 for r in grid if not r.get("control"))
    control = [r for r in grid if r.get("control")]
    assert len(control) == 4 and all(r["seqs"] == 512 and r["n_new"] == 1 for r in control)
    assert set(T.FORWARD_US) == {(d, page) for d in (64, 128) for page in (64, 256)}


def test_statistics_criterion_and_rates():
    row = dict(seqs=16, hk=2, d=128, page=64, fp8=False, n_new=2048)
    times = dict(fused=[10.0, 11.0, 9.0, 10.0, 10.0, 10.0, 10.0], recipe=[20.0, 20.0, 20.0, 22.0, 20.0, 20.0, 20.0])
    s = T.summarise(times, row)
    assert s["fused_us"] == dict(median=10.0, min=9.0, max=11.0, spread=pytest.approx(0.2))
    assert s["recipe_us"]["spread"] == pytest.approx(0.1) and s["recipe_over_fused"] == 2.0
    assert s["twice_the_larger_spread"] == pytest.approx(0.4) and s["fused_beats_recipe"] is True
    # K and V, read as fp16 and written as fp16
    assert T.moved_bytes(row) == 16 * 2 * 2 * 128 * 2048 * 4 == s["fused_bytes"]
    assert s["fused_bytes_per_second"] == pytest.approx(s["fused_bytes"] / 10e-6)
    assert s["fused_share_of_copy_rate"] == pytest.approx(s["fused_bytes_per_second"] / 6.29e12)
    assert T.moved_bytes(dict(row, fp8=True)) == 16 * 2 * 2 * 128 * 2048 * 3
    assert "fused_share_of_forward_paged" not in s
    # a gain inside twice the larger spread does not count, nor does a loss
    assert T.summarise(dict(times, recipe=[13.0] * 7), row)["fused_beats_recipe"] is False
    assert T.summarise(dict(times, recipe=[5.0] * 7), row)["fused_beats_recipe"] is False
    one = T.summarise(times, dict(row, n_new=1))
    assert one["forward_paged_us"] == 99.5 and one["fused_share_of_forward_paged"] == pytest.approx(10.0 / 99.5)
    assert "fused_bytes" not in one
    assert "fused_share_of_forward_paged" not in T.summarise(times, dict(row, n_new=1, control=True))


def test_arguments_and_no_gpu():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "append_time.py"), *a],  # noqa: E731
                                    capture_output=True, text=True, timeout=120)
    r = run("--repeats", "3")
    assert r.returncode == 2 and "at least 5" in r.stderr
    r = run("--only", "64,64")
    assert r.returncode == 2 and "d,page,fp8,n_new" in r.stderr
    r = run("--only", "64,64,0,7")
    assert r.returncode == 2 and "no row" in r.stderr
    if not torch.cuda.is_available():
        r = run()
        assert r.returncode != 0 and "no GPU" in r.stderr
