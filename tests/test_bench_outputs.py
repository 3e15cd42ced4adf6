"""bench.py --dump-outputs and --full.  Host part: dump_outputs writes float64 .npy files of the
last step's solve results and loop state, the whole batch when it is small and a seeded row sample
of the solutions (and, for a large batch, of everything) otherwise, the same rows for the same seed.
GPU part: a plain run times exactly --steps steps, carries none of the --full legs, and two runs
with the same arguments write identical outputs."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

import bench  # noqa: E402

SOLVE = ("x", "y", "status", "iter", "obj_val", "pri_res", "dua_res")
STATE = {"ctrl": 2, "x_true": 4, "xest": 6, "done": 0, "ctrl_seq": 0}
FULL_KEYS = ("cpu_baseline", "config2", "config3", "config4", "n40_accel")


def fake_shard(b0, B, n=5, m=7):
    """a stand-in for one shard of B chasers starting at global id b0: every value names its row"""
    ids = torch.arange(b0, b0 + B, dtype=torch.float64)
    wide = lambda w: ids[:, None] * 100 + torch.arange(w, dtype=torch.float64)  # noqa: E731
    res = types.SimpleNamespace(x=wide(n), y=-wide(m), status=ids.to(torch.int32),
                                iter=(ids * 2).to(torch.int32), obj_val=ids + 0.5,
                                pri_res=ids + 0.25, dua_res=ids + 0.125)
    res.x[0, 0] = float("nan")  # an instance without a solution keeps its NaN
    qp = types.SimpleNamespace(stream=types.SimpleNamespace(synchronize=lambda: None))
    part = types.SimpleNamespace(B=B, qp=qp, device=torch.device("cpu"),
                                 **{k: (wide(w) if w else ids.to(torch.int32)) for k, w in STATE.items()})
    return part, res


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small_batch_is_written_whole(tmp_path):
    parts, results = zip(fake_shard(0, 37), fake_shard(37, 40))
    bench.dump_outputs(str(tmp_path / "a"), parts, results, seed=3)
    a = load_dir(tmp_path / "a")
    assert set(a) == {"rows", "solve_x_nan"} | {f"solve_{k}" for k in SOLVE} | set(STATE)
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["rows"], np.arange(77))
    assert a["solve_x"].shape == (77, 5) and a["solve_y"].shape == (77, 7)
    # finite files: a NaN of the engine is written as 0 and marked in the mask
    assert all(np.isfinite(v).all() for v in a.values())
    nan = np.zeros((77, 5))
    nan[[0, 37], 0] = 1
    assert np.array_equal(a["solve_x_nan"], nan) and a["solve_x"][0, 0] == 0 == a["solve_x"][37, 0]
    assert a["solve_x"][0, 1] == 1 and a["solve_x"][37, 1] == 3701
    assert np.array_equal(a["solve_status"], np.arange(77.0))  # shards in chaser order
    assert np.array_equal(a["solve_iter"], 2 * np.arange(77.0))
    assert np.array_equal(a["x_true"][:, 0], 100 * np.arange(77.0)) and a["x_true"].shape == (77, 4)
    assert a["done"].shape == (77,)


def test_dump_outputs_samples_a_large_batch_by_seed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 16)
    monkeypatch.setattr(bench, "DUMP_FULL_BATCH", 64)
    parts, results = zip(fake_shard(0, 50), fake_shard(50, 49))
    for name, seed in (("a", 3), ("b", 3), ("c", 4)):
        bench.dump_outputs(str(tmp_path / name), parts, results, seed=seed)
    a, b, c = (load_dir(tmp_path / k) for k in "abc")
    rows = a["rows"].astype(int)
    assert len(rows) == 16 and len(set(rows)) == 16 and np.all(np.diff(rows) > 0) and rows.max() < 99
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["rows"], c["rows"])
    own = (rows != 0) & (rows != 50)  # the sampled chasers' own rows (0 and 50 hold the NaN)
    assert np.array_equal(a["solve_x"][own, 0], 100.0 * rows[own])
    assert np.array_equal(a["solve_x"][:, 1], 100.0 * rows + 1)
    # beyond DUMP_FULL_BATCH the per-chaser arrays follow the same sample
    assert np.array_equal(a["solve_status"], rows) and np.array_equal(a["xest"][:, 0], 100.0 * rows)

    monkeypatch.setattr(bench, "DUMP_FULL_BATCH", 128)
    bench.dump_outputs(str(tmp_path / "d"), parts, results, seed=3)
    d = load_dir(tmp_path / "d")
    assert d["solve_x"].shape == (16, 5) and np.array_equal(d["solve_status"], np.arange(99.0))


def test_default_dump_fits_the_size_limit():
    """the default bench (B = 65,536, n = 121, m = 226) and the N = 40 problems (n <= 300,
    m <= 600, at the largest batch written whole) stay below the 64 MB a dump may take"""
    from mpc_arpo_project_amd.closed_loop import BatchClosedLoop

    # the solve's five scalars, the loop state, the run summary and its NaN mask
    per_chaser = 5 + sum(max(w, 1) for w in STATE.values()) + 2 * len(BatchClosedLoop.SUMMARY_FIELDS)
    for B, n, m in ((65536, 121, 226), (bench.DUMP_FULL_BATCH, 300, 600)):
        total = 8 * (bench.DUMP_ROWS * (2 * n + m + 1) + B * per_chaser)  # x, its mask, y, rows
        assert total < 64e6, (B, total)


def run_bench(capsys, *argv):
    assert bench.main(["bench.py", *argv]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_repeats_its_outputs(tmp_path, capsys):
    # 301 chasers on two shards (150 + 151): odd, and more than one workgroup per launch
    args = ("--gpus", "1", "--batch", "301", "--steps", "3", "--warmup", "2")
    a = run_bench(capsys, *args, "--dump-outputs", str(tmp_path / "a"))
    b = run_bench(capsys, *args, "--dump-outputs", str(tmp_path / "b"))
    for out in (a, b):
        assert out["steps"] == 3 and out["warmup"] == 2 and out["unit"] == "solves/s"
        assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["metric"]
        assert out["ms_per_step"] > 0
        assert out["solves"]["offered"] == 3 * 301  # three timed steps, no more
        assert out["value"] == pytest.approx(out["solves"]["counted"] / (3 * out["ms_per_step"] * 1e-3))
        assert not [k for k in FULL_KEYS if k in out], "a plain run carries no --full leg"
    da, db = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert set(da) == ({"rows", "summary", "summary_nan", "solve_x_nan"} |
                       {f"solve_{k}" for k in SOLVE} | set(STATE))
    assert sum(v.nbytes for v in da.values()) < 64e6
    for k, v in da.items():
        assert v.dtype == np.float64 and v.shape[0] == 301, k
        assert np.isfinite(v).all() and np.array_equal(v, db[k]), k
    assert da["solve_x"].shape[1] == 121 and da["solve_y"].shape[1] == 226
    solved = da["solve_status"] == 1
    assert solved.any() and not da["solve_x_nan"][solved].any()
    assert np.all(da["solve_iter"][solved] > 0)
    assert da["summary"].shape == (301, 9)
