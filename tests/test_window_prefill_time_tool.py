"""CPU test of tools/window_prefill_time.py's plumbing: the grid it times, the statistics, the
ratios and the acceptance condition it derives from the windows' times, the record's schema, its argument checks, and
that it refuses to run without a GPU."""

import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import window_prefill_time as T  # noqa: E402


def test_the_grid_is_the_issues_without_the_delegated_combinations():
    grid = T.shapes()
    main = [(s["g"], s["nq"], s["d"], s["window"]) for s in grid if not s.get("control")]
    want = [(g, nq, d, w) for d in (64, 128) for g in (1, 4, 8) for nq in (128, 512, 2048) for w in (1024, 4096)
            if g * nq > 128]
    assert main == want and len(main) == 32
    assert all(s["seqs"] == 16 and s["hk"] == 2 for s in grid if not s.get("control"))
    control = [s for s in grid if s.get("control")]
    assert [(s["seqs"] * s["hk"], s["g"], s["nq"], s["d"], s["window"]) for s in control] == [(1024, 4, 128, 64, 1024),
                                                                                               (1024, 4, 128, 128, 1024)]
    assert T.CAP == 16384 and T.PAGES == (64, 256)
    for s in grid:
        for page in T.PAGES:
            launched, chunk, span_w, cap_chunks, pb, rows, nqb, delegated = T.plan(s["g"], s["nq"], T.CAP, s["d"], page, s["window"])
            assert not delegated and nqb >= 2 and s["nq"] % pb == 0 and span_w == s["window"] + pb - 1
            assert 1 <= launched <= cap_chunks and cap_chunks * chunk >= T.CAP
            assert not T.plan(s["g"], s["nq"], T.CAP, s["d"], page, T.CAP - 1)[7]  # (c) is not delegated


def test_statistics_ratios_and_condition():
    times = dict(window_prefill=[1.0, 1.1, 0.9, 1.0, 1.0, 1.0, 1.0], loop=[2.0, 2.0, 2.0, 2.2, 2.0, 2.0, 2.0],
                 loop_copy=[3.0] * 7, prefill=[4.0] * 7, window_cap=[4.2] * 7)
    s = T.summarise(times, 4)
    assert set(s) == {r + "_ms" for r in T.RUNS} | {"loop_over_window_prefill", "loop_copy_over_window_prefill",
                                                     "prefill_over_window_prefill", "window_cap_over_prefill",
                                                     "run_to_run_spread", "not_slower_than_loop", "condition_applies"}
    assert s["window_prefill_ms"] == dict(median=1.0, min=0.9, max=1.1, spread=pytest.approx(0.2))
    assert s["loop_ms"]["spread"] == pytest.approx(0.1) and s["loop_copy_ms"]["spread"] == 0.0
    assert s["loop_over_window_prefill"] == 2.0 and s["loop_copy_over_window_prefill"] == 3.0
    assert s["prefill_over_window_prefill"] == 4.0 and s["window_cap_over_prefill"] == pytest.approx(1.05)
    assert s["run_to_run_spread"] == pytest.approx(0.2)
    assert s["not_slower_than_loop"] is True and s["condition_applies"] is True
    # slower by less than the spread still passes, slower by more does not; fewer than 4 blocks: not required
    assert T.summarise(dict(times, loop=[0.9] * 7), 4)["not_slower_than_loop"] is True
    assert T.summarise(dict(times, loop=[0.5] * 7), 4)["not_slower_than_loop"] is False
    assert T.summarise(times, 3)["condition_applies"] is False


def test_the_file_holds_every_field_once_and_load_gives_the_cases_back(tmp_path):
    times = dict(window_prefill=[1.0, 1.1, 0.9, 1.0, 1.0], loop=[2.0] * 5, loop_copy=[3.0] * 5, prefill=[4.0] * 5,
                 window_cap=[4.123456] * 5)
    case = dict(kv_group=4, nq=512, d=64, window=1024, page=64, lengths="full", control=False,
                calls_per_window=dict(loop=7), **T.summarise(times, 16))
    slow = dict(case, lengths="random", not_slower_than_loop=False)
    path = str(tmp_path / "t.json")
    T.write_out(path, dict(device="x", repeats=5, window_ms=20.0), [case, slow])
    with open(path) as f:
        text = f.read()
    data = json.loads(text)
    assert len(text.splitlines()) == 2 + 2 and text.count("loop_over_window_prefill") == 1
    assert data["device"] == "x" and "window_cap_ms.median" in data["fields"] and "calls_per_window.loop" in data["fields"]
    assert data["cases_that_miss_the_condition"] == [[4, 512, 64, 1024, 64, "random", False]]
    assert "the FP8 pools" in data["not_measured"]
    back = T.load(path)
    assert back[0]["window_cap_ms"]["median"] == 4.123 and back[0]["calls_per_window"] == dict(loop=7)
    assert set(back[0]) == set(case) and back[1]["not_slower_than_loop"] is False
    committed = T.load(os.path.join(ROOT, "profiles", "window_prefill_time.json"))
    assert len(committed) == 136 and set(committed[0]) >= set(T.summarise(times, 4))


def test_arguments_and_no_gpu():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "window_prefill_time.py"), *a],  # noqa: E731
                                    capture_output=True, text=True, timeout=120)
    r = run("--repeats", "3")
    assert r.returncode == 2 and "at least 5" in r.stderr
    r = run("--only", "4,512,64")
    assert r.returncode == 2 and "g,nq,d,W" in r.stderr
    if not torch.cuda.is_available():
        r = run()
        assert r.returncode != 0 and "no GPU" in r.stderr
