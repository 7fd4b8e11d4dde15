"""bench.py's options and its --dump-outputs writer, without a GPU."""
import numpy as np

import bench


def test_a_plain_run_times_one_block_of_exactly_the_steps():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not args.full and args.dump_outputs is None
    assert bench.timed_blocks(args, t_step=1e-5) == 1
    assert bench.timed_blocks(bench.parse_args(["--steps", "7", "--repeats", "4"]), t_step=1e-5) == 4


def test_full_keeps_the_timed_blocks_up_to_min_seconds():
    args = bench.parse_args(["--steps", "100", "--full", "--min-seconds", "2"])
    assert args.full
    assert bench.timed_blocks(args, t_step=1e-3) == 20               # 2 s / (100 x 1 ms)
    assert bench.timed_blocks(args, t_step=1.0) == 3                 # never fewer than 3 blocks


def test_dump_outputs_writes_float64_whole_arrays_under_the_limit(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = np.linspace(0.0, 1.0, 5)
    bench.write_outputs(str(tmp_path / "out"), {"a": a, "b": b})
    ga, gb = np.load(tmp_path / "out" / "a.npy"), np.load(tmp_path / "out" / "b.npy")
    assert ga.dtype == np.float64 and np.array_equal(ga, a)
    assert gb.dtype == np.float64 and np.array_equal(gb, b)


def test_dump_outputs_samples_the_same_rows_when_over_the_limit(tmp_path):
    rows = np.arange(1000, dtype=np.float64)[:, None] * np.ones((1, 16))          # 128 kB; row i holds i
    flat = np.arange(3000, dtype=np.float64)                                      # 24 kB
    limit = 40_000
    for d in ("one", "two"):
        bench.write_outputs(str(tmp_path / d), {"rows": rows, "flat": flat}, limit_bytes=limit)
    r1, r2 = np.load(tmp_path / "one" / "rows.npy"), np.load(tmp_path / "two" / "rows.npy")
    f1 = np.load(tmp_path / "one" / "flat.npy")
    assert np.array_equal(r1, r2)                                    # a fixed, seeded sample
    assert r1.nbytes + f1.nbytes <= limit
    assert 0 < len(r1) < 1000 and 0 < len(f1) < 3000
    idx = r1[:, 0]
    assert np.all(np.diff(idx) > 0) and np.array_equal(r1, rows[idx.astype(int)])   # whole rows, in order
    assert np.all(np.diff(f1) > 0) and np.all(np.isin(f1, flat))


def test_dump_outputs_keeps_the_limit_whatever_the_shapes(tmp_path):
    wide = np.arange(8000, dtype=np.float64).reshape(1, 8000)                    # one row larger than its share
    flat = np.arange(2000, dtype=np.float64)
    scalar = np.array(3.0)
    limit = 20_000
    bench.write_outputs(str(tmp_path), {"wide": wide, "flat": flat, "scalar": scalar}, limit_bytes=limit)
    got = {k: np.load(tmp_path / (k + ".npy")) for k in ("wide", "flat", "scalar")}
    assert sum(g.nbytes for g in got.values()) <= limit
    w = got["wide"]
    assert w.ndim == 1 and 0 < len(w) < 8000 and np.all(np.diff(w) > 0) and np.all(np.isin(w, wide))
    assert 0 < len(got["flat"]) < 2000
