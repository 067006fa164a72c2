"""bench.py's command line and output dump, without a GPU: a plain run carries none of the legs that take runs of
their own (they need --full), and --dump-outputs writes a deterministic float64 view of the fired results within
its byte budget."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extra_legs(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert [getattr(a, leg) for leg in bench.FULL_LEGS] == [0] * len(bench.FULL_LEGS)
    assert a.no_check
    # switching a leg off explicitly stays valid without --full; asking for one does not
    a = _parse(bench, monkeypatch, "--prof-steps", "0", "--cpu-sample", "0", "--drain-steps", "0")
    assert a.prof_steps == 0 and a.drain_steps == 0
    with pytest.raises(SystemExit):
        _parse(bench, monkeypatch, "--drain-steps", "4")


def test_full_run_keeps_the_legs_defaults(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--full")
    assert {leg: getattr(a, leg) for leg in bench.FULL_LEGS} == bench.FULL_LEGS
    assert not a.no_check
    a = _parse(bench, monkeypatch, "--full", "--decode-steps", "0", "--h2d-steps", "2", "--dump-outputs", "d")
    assert (a.decode_steps, a.h2d_steps, a.prof_steps, a.dump_outputs) == (0, 2, bench.FULL_LEGS["prof_steps"], "d")


def _fired(rng, n, windows):
    return {"n": n, "key": rng.integers(0, 1 << 16, n), "f1": rng.integers(0, 1 << 40, n),
            "ts": 1_700_000_000_999 + 1000 * rng.integers(0, windows, n),
            "sum_i64": rng.integers(-(1 << 63), (1 << 63) - 1, n), "count": None, "win_start": None, "sum_f64": None}


def test_dump_outputs_is_float64_sorted_and_order_independent(bench, tmp_path):
    res = _fired(np.random.default_rng(1), 5000, 3)
    perm = np.random.default_rng(2).permutation(res["n"])
    shuffled = {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), shuffled)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["f1.npy", "key.npy", "sum_i64.npy", "sum_i64_lo32.npy", "ts.npy"] == sorted(os.listdir(tmp_path / "b"))
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n[:-4]].dtype == np.float64 and np.array_equal(a[n[:-4]], np.load(tmp_path / "b" / n))
    # everything fits the budget here: every row, ordered by (ts, key), sums exact through their low words
    order = np.lexsort([res["sum_i64"], res["f1"], res["key"], res["ts"]])
    assert np.array_equal(a["ts"], res["ts"][order]) and np.array_equal(a["key"], res["key"][order])
    assert np.array_equal(a["sum_i64_lo32"], (res["sum_i64"][order].view(np.uint64) & np.uint64(0xFFFFFFFF)))
    assert np.array_equal(a["sum_i64"], res["sum_i64"][order].astype(np.float64))


def test_dump_outputs_keeps_the_latest_windows_within_its_budget(bench, tmp_path, monkeypatch):
    res = _fired(np.random.default_rng(3), 6000, 4)
    per_window = np.bincount((res["ts"] - res["ts"].min()) // 1000)
    row_bytes = 8 * 5
    # room for the two latest windows but not the third
    monkeypatch.setattr(bench, "DUMP_BYTES", row_bytes * int(per_window[-1] + per_window[-2] + 1))
    bench.dump_outputs(str(tmp_path / "two"), res)
    ts = np.load(tmp_path / "two" / "ts.npy")
    assert len(ts) == per_window[-1] + per_window[-2] and set(ts) == set(np.unique(res["ts"])[-2:].astype(np.float64))
    # less than one window: a fixed sample of the latest one, the same on every run
    monkeypatch.setattr(bench, "DUMP_BYTES", row_bytes * 100)
    bench.dump_outputs(str(tmp_path / "s1"), res)
    bench.dump_outputs(str(tmp_path / "s2"), res)
    for n in os.listdir(tmp_path / "s1"):
        x = np.load(tmp_path / "s1" / n)
        assert len(x) == 100 and np.array_equal(x, np.load(tmp_path / "s2" / n))
    assert set(np.load(tmp_path / "s1" / "ts.npy")) == {float(res["ts"].max())}
    assert sum(os.path.getsize(tmp_path / "s1" / n) for n in os.listdir(tmp_path / "s1")) <= row_bytes * 100 + 5 * 128


def test_dump_outputs_of_nothing_fired(bench, tmp_path):
    empty = {"n": 0, **{c: np.zeros(0, np.float64 if c.endswith("f64") else np.int64) for c in bench.OUT_COLUMNS}}
    bench.dump_outputs(str(tmp_path / "e"), empty)
    assert all(len(np.load(tmp_path / "e" / n)) == 0 for n in os.listdir(tmp_path / "e"))
