"""bench.py's launch contract, checked without a GPU: `--gpus N` on a node with fewer than N devices must fail loudly
(not report n_gpus = 1), and under torchrun a WORLD_SIZE that disagrees with --gpus is an error too; the line, --full and
--dump-outputs (one test marked gpu runs a plain benchmark)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=300)


def test_more_gpus_than_devices_is_an_error():
    r = _run(["--gpus", "2", "--steps", "1"])
    assert r.returncode != 0
    assert "needs 2 devices" in r.stderr and '"n_gpus"' not in r.stdout


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2", "--steps", "1"], {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr and '"n_gpus"' not in r.stdout


def test_pool_flag_is_for_pool_workloads():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert {"c1", "c2", "c3", "c4", "c5"} <= set(m.WORKLOADS)
    assert m.WORKLOADS["c5"]["picks"] == 100 and m.WORKLOADS["c4"]["score"] == "MPE"
    assert m.SPLIT_PRODUCTS == {"p2": 3, "h2": 3, "bf3": 6}


def _bench_mod():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_compact_line_fits_the_driver_tail():
    """The line the driver parses: built by the same function main() prints through, from full records of every workload
    (round 5's 17-22 KB lines are the canned results), must be ONE line of at most 4 096 characters, strict JSON, and
    carry the contract's fields, the roofline and the CPU baseline."""
    import glob
    import json

    m = _bench_mod()
    recs = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "bench_records", "*.json")))
    assert len(recs) >= 4
    for p in recs:
        with open(p) as f:
            full = json.load(f)
        line = m.compact_line(full, "bench_detail.json")
        assert "\n" not in line and len(line) <= 4096, (p, len(line))
        d = json.loads(line, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))  # strict: no NaN / Infinity
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline"):
            assert k in d, (p, k)
        assert d["value"] == round(full["value"], 4) and d["ms_per_step"] == round(full["ms_per_step"], 4)
        assert len(d["dtype"]) <= 120 and "workload" in d["config"]
        r = d["roofline"]
        if r is not None:
            assert set(("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r) and len(r["kernel"]) <= 60
            if r["frac"] is not None:
                assert abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
        if "cpu_baseline" in full:
            cb = d["cpu_baseline"]
            assert set(("value", "unit", "cores", "kind", "sample", "parity_sample")) <= set(cb)
            assert all(isinstance(x, (int, float, bool)) for x in cb["parity_sample"].values())
        if "companions" in full:
            for name in ("c3", "c4", "c2_with_input"):
                assert set(("ms_per_step", "value", "frac")) <= set(d["companions"][name])
        if "exact_modes" in full:
            assert set(d["exact_modes"]) == {"h2", "bf3", "fp32"}


def test_compact_line_survives_non_finite_and_oversized_input():
    import json

    m = _bench_mod()
    full = {"metric": "m", "value": float("nan"), "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": float("inf"),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 " + "x" * 500, "data": "synthetic",
            "config": {"workload": "w" * 1000, "parallelism": "p" * 400},
            "roofline": {"kernel": "k" * 900, "bound": "hbm", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 1.25e-4, "traffic": None,
                         "other_kernels": [{"kernel": "z" * 5000}] * 40},
            "companions": {n: {"error": "e" * 2000} for n in ("c3", "c4", "c2_with_input")},
            "attribution": {"per_rank_s": {"min": 1, "mean": 1, "max": 1, "all": [1.0] * 64}, "compute_s": {"min": 1, "max": 2}}}
    line = m.compact_line(full, "d.json")
    assert len(line) <= 4096
    d = json.loads(line)
    assert d["value"] is None and d["ms_per_step"] is None and len(d["roofline"]["kernel"]) <= 60 and "all" not in d["attribution"]["per_rank_s"]


def test_full_and_dump_outputs_are_options():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files only, at most 64 MB in all; an array larger than its share is replaced by the
    same seeded sample of its elements on every call."""
    import numpy as np
    import torch

    m = _bench_mod()
    rng = np.random.default_rng(3)
    arrays = {"big": rng.standard_normal(20_000_000).astype(np.float32),  # 80 MB: sampled
              "kp": torch.from_numpy(rng.standard_normal((4, 19, 3))),
              "idx": torch.arange(10, dtype=torch.int64), "mask": np.array([True, False]), "half": torch.ones(3, dtype=torch.float16)}
    for d in ("a", "b"):
        m.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    assert total <= 64_000_000 and total > 60_000_000
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "kp.npy"), arrays["kp"].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "idx.npy"), np.arange(10, dtype=np.float64))
    assert np.load(tmp_path / "a" / "half.npy").dtype == np.float32
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.ndim == 1 and 10_000_000 < big.size < arrays["big"].size and np.isin(big[:100], arrays["big"]).all()


@pytest.mark.gpu
def test_plain_run_times_exactly_k_steps_and_dumps_outputs(tmp_path):
    """A plain run: the contract fields, exactly --steps timed steps, none of the --full measurements, and --dump-outputs writes the last
    step's heat-maps and triangulation results -- the same values on a second run with the same arguments."""
    import json

    import numpy as np

    lines = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        ls = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(ls) == 1
        lines.append(json.loads(ls[0]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert d[k] is not None, k
    assert d["steps"] == 3 and d["timed_repeats"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["roofline"] is None and not ({"cpu_baseline", "exact_modes", "companions", "detail"} & set(d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert {"heatmaps.npy", "keypoints_3d.npy", "keypoints_2d.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    hm = np.load(tmp_path / "a" / "heatmaps.npy")
    assert hm.dtype == np.float32 and hm.shape == (32, 4, 19, 64, 64) and np.isfinite(hm).all()
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=f)
