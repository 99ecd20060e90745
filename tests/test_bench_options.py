"""bench.py's run modes and --dump-outputs helpers (host side, no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--dump-outputs", "somewhere")
    assert a.full and a.no_cpu_baseline and a.dump_outputs == "somewhere"
    assert _parse(monkeypatch, "--full", "--check").check


@pytest.mark.parametrize("argv", [["--check"], ["--steps", "0"]])
def test_arguments_a_run_cannot_honour_are_refused(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True)
    assert r.returncode == 2 and "bench.py: error" in r.stderr


def test_dump_sample_is_fixed_sorted_and_named():
    import torch
    import bench
    x = torch.arange(5000, dtype=torch.int32)
    assert bench._dump_pick(torch, x, 5000, "a") is x  # small outputs are written whole
    a, b = bench._dump_pick(torch, x, 64, "a"), bench._dump_pick(torch, x, 64, "a")
    assert a.numel() == 64 and torch.equal(a, b) and bool((a[1:] >= a[:-1]).all())
    assert not torch.equal(a, bench._dump_pick(torch, x, 64, "b"))


def test_dump_class_rows_skips_the_unwritten_gaps():
    import torch
    import bench

    class Rows:
        off = torch.tensor([0, 5, 9, 12, 20], dtype=torch.int64)  # capacity-based offsets
        ln = torch.tensor([2, 0, 3, 1], dtype=torch.int32)        # used lengths
        nbr = torch.arange(100, 120, dtype=torch.int32)
        wpk = torch.arange(200, 220, dtype=torch.int32)
    nbr, wpk = bench._dump_class_rows(torch, Rows, 4)
    assert nbr.tolist() == [100, 101, 109, 110, 111, 112] and wpk.tolist() == [200, 201, 209, 210, 211, 212]
    assert bench._dump_class_rows(torch, Rows, 3)[0].tolist() == [100, 101, 109, 110, 111]


def test_ring_slots_name_the_last_set_of_every_buffer():
    import bench
    info = np.arange(16)
    got = bench.ring_slots(3, 16, lambda t: 10 * t, "abc", "xyz", info)
    assert got == [(0, 150, "a", "x", 15), (1, 130, "b", "y", 13), (2, 140, "c", "z", 14)]
    assert [s[:2] for s in bench.ring_slots(4, 2, lambda t: t, "abcd", "wxyz", info)] == [(0, 0), (1, 1)]
