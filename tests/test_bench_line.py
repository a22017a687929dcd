"""bench.py's ONE stdout line stays inside what the driver captures (round 5's 20.9 KB line was cut at
~8 KB and the round's measurement was lost).  CPU: the compaction on the committed full records of earlier rounds and on an
inflated record; GPU: the real script end to end."""
import glob
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline")
ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic")
CPU = ("value", "unit", "cores", "kind", "sample")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _check(line, full, limit):
    assert "\n" not in line
    assert len(line.encode()) <= limit, len(line)
    d = json.loads(line)
    for k in CONTRACT:
        assert k in d, k
    assert d["config"]["workload"]
    assert abs(d["value"] - full["value"]) <= 1e-4 * abs(full["value"])
    assert abs(d["ms_per_step"] - full["ms_per_step"]) <= 1e-4 * abs(full["ms_per_step"])
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "dtype", "scaling", "higher_is_better", "data"):
        assert d[k] == full[k], k
    if full.get("roofline"):
        for k in ROOFLINE:
            assert k in d["roofline"], k
        assert abs(d["roofline"]["frac"] - full["roofline"]["frac"]) <= 1e-4
        assert abs(d["roofline"]["achieved"] / d["roofline"]["peak"] - d["roofline"]["frac"]) <= 1e-3
    if full.get("cpu_baseline"):
        for k in CPU:
            assert k in d["cpu_baseline"], k
    return d


def test_committed_full_records_compact_under_the_limit():
    b = _bench()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench_cfg*.json")))
    assert len(files) >= 10
    seen_other = False
    for f in files:
        txt = open(f).read().strip()
        if not txt.startswith("{"):
            continue
        full = json.loads(txt.splitlines()[-1])
        if "value" not in full or full.get("value") is None:
            continue
        line = b.compact_line(full, "bench_details.json")
        d = _check(line, full, b.LINE_LIMIT)
        if "other_configs" in full:
            seen_other = True
            assert set(d["other_configs"]) == set(full["other_configs"])     # every BASELINE config still on the line
            assert d["other_configs"]["cfg4"]["value"] > 0
            assert len(d["other_configs"]["cfg5"]["renders"]) == len(full["other_configs"]["cfg5"]["renders"])
    assert seen_other


def test_an_inflated_record_drops_optional_parts_never_contract_keys():
    b = _bench()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r05_bench_cfg3_driver_args_20frames.json")).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 20000          # the line that was lost
    big = json.loads(json.dumps(full))
    big["other_configs"]["cfg5"]["renders"] = big["other_configs"]["cfg5"]["renders"] * 40
    big["roofline"]["limiter"] = "x" * 5000
    big["cpu_baseline"]["sample"] = "y" * 5000
    big["config"]["workload"] = "cfg3: " + "z" * 3000
    line = b.compact_line(big, "bench_details.json")
    d = _check(line, big, b.LINE_LIMIT)
    assert "other_configs" not in d and "roofline_stages" in d
    # a tighter limit drops more, still valid
    line = b.compact_line(big, None, limit=2500)
    _check(line, big, 2500)


def test_details_file_round_trips(tmp_path):
    b = _bench()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r05_bench_cfg3_driver_args_20frames.json")).read().strip().splitlines()[-1])
    p = b.write_details(full, str(tmp_path / "sub" / "details.json"))
    assert p and json.load(open(p)) == full


def test_frame_plan_times_exactly_the_steps_and_bounds_the_map():
    """one pass -- the last K frames of the workload's stream, as ever -- while K + W fit the map; beyond it passes of the last
    frames of a stream no longer than the map may be, whose timed frames add up to K"""
    b = _bench()
    assert b.frame_plan("cfg3", 20, 5) == (300, 275, [20])
    assert b.frame_plan("cfg3", 295, 5) == (300, 0, [295])
    assert b.frame_plan("cfg3", 100, 5, 0) == (105, 0, [100])
    assert b.frame_plan("cfg4", 40, 5) == (45, 0, [40])
    assert b.frame_plan("cfg3", 100, 5, 400) == (400, 295, [100])
    for wl, cap in b.MAX_MAP_FRAMES.items():
        for k, w in ((cap, 5), (cap + 1, 0), (2000, 5), (22222, 5), (5000, 1)):
            total, pre, passes = b.frame_plan(wl, k, w)
            assert sum(passes) == k and total <= cap and pre == 0 and len(passes) > 1
            assert all(0 < n <= total - w for n in passes)


@pytest.mark.gpu
def test_real_bench_output_is_one_short_parseable_line(tmp_path):
    det = str(tmp_path / "details.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-budget", "1",
                        "--repeats", "2", "--full", "--no-other-configs", "--details", det], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    assert len(lines[0].encode()) <= 6000
    d = json.loads(lines[0])
    full = json.load(open(det))
    _check(lines[0], full, 6000)
    assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """a plain run (no --full) times exactly --steps frames and, with --dump-outputs, writes the last timed frame's image, pose and
    map sample as float32 / float64 .npy files (< 64 MB); two runs with the same arguments write identical arrays"""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--repeats", "1",
                            "--map-frames", "0", "--details", "", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines[:3]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-2 * 1e3
        assert line["cpu_baseline"] is None and "other_configs" not in line
        files = sorted(p.name for p in d.iterdir())
        assert files == ["image.npy", "pool_nodes.npy", "pool_sample_index.npy", "pool_sample_words.npy", "pose_orientation.npy",
                         "pose_position.npy"], files
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 << 20
        arrs = {f[:-4]: np.load(str(d / f)) for f in files}
        for a in arrs.values():
            assert a.dtype in (np.float32, np.float64)
        assert arrs["image"].shape == (480, 640, 4)
        assert arrs["pool_nodes"][0] > 0 and arrs["pool_sample_words"].shape == (len(arrs["pool_sample_index"]), 2)
        dumps.append(arrs)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


@pytest.mark.gpu
def test_plain_run_with_more_steps_than_one_map_holds(tmp_path):
    """--steps beyond the frames one map may hold: the steps are timed in passes, all of them counted"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "700", "--warmup", "5", "--repeats", "2",
                        "--details", ""], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    line = json.loads(lines[0])
    assert line["steps"] == 700 and line["warmup"] == 5 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-2 * 1e3
    assert line["config"]["frames_in_map_at_end"] == 300 and len(line["runs"]) == 2
