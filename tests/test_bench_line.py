"""bench.py's final stdout line must stay parseable by the driver, which keeps ~9 KB of stdout tail (round 4's 25.9 KB line left
BENCH_r04.parsed null).  CPU: the compaction on a committed full record, on a bloated synthetic one, and on the --dry path; the
--dump-outputs writer and option checks.  GPU: a plain run's line and the detections it dumps."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config")


def test_compact_line_of_a_real_full_record_is_short_and_keeps_what_is_judged():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default_line_run2.json")))      # 25.9 KB: the line that did not parse
    assert len(json.dumps(full)) > 20000
    line = b.compact_line(full, "gpurun_out/bench_full_detect_n1.json")
    assert len(line) < b.LINE_MAX <= 8000 and "\n" not in line
    d = json.loads(line)
    for k in CONTRACT:
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"] and d["steps"] == 20 and d["warmup"] == 5
    assert d["config"]["workload"].startswith("detection-mode infer_simple") and d["config"]["volumes_per_step"] == 4
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "frac_algorithmic", "kernel_ms", "traffic"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-5
    assert set(d["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"} and d["cpu_baseline"]["kind"] == "port"
    for sub in ("configs1_backbone", "stress_rois", "configs3_prm_soma", "prm_nuclei_tile", "volume_pipeline"):
        r = d[sub]
        assert r["value"] > 0 and r["ms_per_step"] > 0 and "workload" in r["config"]
        assert "roofline" in r and (r["roofline"] is None or "frac" in r["roofline"])
    assert "rooflines" not in d and "step_ms_timed" not in json.dumps(d) and "frac_definition" not in line


def test_compact_line_survives_a_bloated_record_and_non_finite_numbers():
    b = _bench()
    blob = "x" * 5000
    rec = {"metric": b.METRIC, "value": 1.0, "unit": "voxels/s", "n_gpus": 8, "steps": 3, "warmup": 1, "ms_per_step": float("nan"),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": blob, "volumes_per_step": 64, "backend": "nccl", "junk": [1] * 4000},
           "roofline": {"bound": "mfma", "kernel": blob, "achieved": float("inf"), "peak": 157.3, "unit": "TFLOP/s", "frac": 0.5,
                        "frac_definition": blob, "traffic": None},
           "cpu_baseline": {"value": 2.0, "unit": "voxels/s", "cores": 16, "kind": "port", "sample": blob, "more": blob},
           "exchange": {"us": 31.5, "ranks": 8, "backend": "nccl", "what": blob},
           "without_exchange": {"value": 3.0, "ms_per_step": 4.0, "what": blob}}
    for k in ("configs1_backbone", "stress_rois", "configs3_prm_soma", "prm_nuclei_tile", "volume_pipeline"):
        rec[k] = {"value": 5.0, "ms_per_step": 6.0, "roofline": {"bound": "hbm", "kernel": blob, "frac": 0.1, "traffic": 7.0, "note": blob},
                  "cpu_baseline": {"value": 1.0, "cores": 16, "kind": "port", "sample": blob}, "config": {"workload": blob, "phase_ms": {"a": 1.0}},
                  "volumes": {"nuclei": {"value": 1.0, "seconds_per_volume": 2.0, "peaks": 3, "cpu_baseline": {"sample": blob}}}}
    rec["prm_nuclei_tile"] = {"error": blob}
    line = b.compact_line(rec)
    assert len(line) < 8000
    d = json.loads(line)                                   # strict JSON: no NaN / Infinity tokens
    assert "NaN" not in line and "Infinity" not in line
    assert d["ms_per_step"] is None and d["roofline"]["achieved"] is None
    assert d["exchange"] == {"us": 31.5, "ranks": 8, "backend": "nccl"} and d["n_gpus"] == 8
    assert d["without_exchange"] == {"value": 3.0, "ms_per_step": 4.0}
    assert len(d["prm_nuclei_tile"]["error"]) <= 200


def test_dry_run_prints_one_short_json_line_last():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.rstrip("\n").splitlines()[-1]
    assert len(last) < 8000
    d = json.loads(last)
    for k in CONTRACT:
        assert k in d, k
    assert d["dry"] is True and d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1


def test_a_hardware_fraction_above_one_is_an_accounting_error():
    """Round 5's soma volume counted peaks the engine had skipped (frac 1.89): the checker must flag that record, pass the newest
    committed one, and emit() must carry the finding on the line."""
    b = _bench()
    r05 = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default_full_record.json")))
    bad = b.hardware_fracs_above_one(r05)
    assert any("volume_pipeline" in p and "soma" in p and v > 1.5 for p, v in bad), bad
    assert b.hardware_fracs_above_one({"roofline": {"frac": 0.63, "frac_algorithmic": 1.76}, "rooflines": [{"frac": 1.0}]}) == []
    assert b.hardware_fracs_above_one({"a": [{"roofline": {"frac": 1.2}}]}) == [("a[0].roofline.frac", 1.2)]
    import glob
    newest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r06_bench_default_full_record*.json")))
    for f in newest:                                       # this round's judged copies: no fraction above 1 anywhere
        rec = json.load(open(f))
        assert b.hardware_fracs_above_one(rec) == [], f
        soma = rec["configs3_prm_soma"]["config"]
        assert soma["peaks_back_propagated"] == soma["peaks_per_tile"], soma
    line = json.loads(b.compact_line(dict(r05, accounting_errors=["%s = %.3f > 1" % x for x in bad])))
    assert line["accounting_errors"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}


def test_dump_outputs_writes_float32_and_a_fixed_sample_of_an_array_beyond_its_share(tmp_path, monkeypatch):
    import numpy as np
    import torch
    b = _bench()
    small = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    big = torch.arange(4096, dtype=torch.float64)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 2048)                     # 1 KB per array
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.numpy())
    g = np.load(tmp_path / "a" / "big.npy")
    assert g.dtype == np.float32 and g.shape == (256,) and np.all(np.diff(g) > 0)      # distinct elements in index order
    assert np.array_equal(g, np.load(tmp_path / "b" / "big.npy"))


def test_options_outside_their_workload_are_refused():
    bench = os.path.join(ROOT, "bench.py")
    for extra in (["--dry", "--dump-outputs", "x"], ["--workload", "prm", "--dump-outputs", "x"], ["--interleaved"], ["--pipelined"]):
        r = subprocess.run([sys.executable, bench, "--steps", "1"] + extra, capture_output=True, text=True, timeout=120, env=_env())
        assert r.returncode == 2 and "error:" in r.stderr, (extra, r.stderr[-500:])


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_steps_detections(tmp_path):
    import numpy as np
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
    for k in CONTRACT:
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "voxels/s" and d["dtype"] == "f32"
    assert abs(d["value"] - 4 * 128 ** 3 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert not set(d) & {"roofline", "cpu_baseline", "resident", "sustained", "configs1_backbone", "volume_pipeline", "full_record"}
    det = np.load(out / "detections.npy")
    assert det.dtype == np.float32 and det.shape == (1, 4, 301, 7)
    counts = det[0, :, 300, 0]
    assert np.all(counts == np.round(counts)) and np.all(counts >= 0) and np.all(counts <= 300) and counts.sum() > 0
    assert abs(float(counts.mean()) - d["config"]["dets_per_volume"]) < 1e-6
