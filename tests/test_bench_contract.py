"""bench.py's launch contract: `--gpus N` must really run N ranks or refuse."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_refuses_more_gpus_than_visible():
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    r = _run(["--gpus", str(n + 1), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "GPU(s)" in r.stderr and not r.stdout.strip()


def test_refuses_world_size_mismatch():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


@pytest.mark.gpu
def test_plain_invocation_with_two_gpus_runs_two_rccl_ranks():
    """`python bench.py --gpus 2` with no launcher: bench.py spawns the ranks itself, the JSON line reports the ranks
    the communicator saw.  Needs a box with >= 2 GPUs (the gpurun boxes have one: skipped there)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    r = _run(["--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and len(line["devices"]) == 2


@pytest.mark.gpu
def test_train_mode_executes_the_rccl_exchange_on_one_gpu():
    """IAF_BENCH_FORCE_DIST=1: a one-rank RCCL communicator, so the bucketed all-reduce path of --train really runs on
    the hardware that is there (the exchange is reported as executed, with its own timing)"""
    r = _run(["--train", "--steps", "3", "--warmup", "1", "--depths", "2,2"], {"IAF_BENCH_FORCE_DIST": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rccl_ranks"] == 1 and line["exchange"]["executed"] is True
    assert line["exchange"]["buckets"] >= 2 and line["exchange"]["alone_ms"] > 0


@pytest.mark.gpu
def test_default_line_carries_the_widened_modes_and_the_settle_count():
    """VERDICT r05 "next" #3: the driver only runs `python bench.py`, so that line carries the other SURVEY 8f rows (`modes`: the training
    step of the whole model, its forward, one importance-sample pass, the posterior block), the untimed settle replays as a key of their
    own, and the two objects of the measurement contract"""
    r = _run(["--steps", "20", "--warmup", "2", "--repeats", "2"], timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "samples/s" and line["n_gpus"] == 1 and line["vs_baseline"] is None
    assert isinstance(line["config"]["settle_replays"], int) and line["config"]["settle_replays"] >= 0
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert 0 < line["roofline"]["frac"] < 1 and line["roofline"]["peak"] == pytest.approx(2500.0 / 6.0)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    m = line["modes"]
    for k in ("train_model_ms", "model_fwd_ms", "iw_eval_ms_per_pass", "posterior_block_us_16x16", "posterior_block_us_8x8"):
        assert isinstance(m.get(k), float) and m[k] > 0, (k, m.get(k))
    assert 0 < m["train_model_frac"] < 1


@pytest.mark.gpu
def test_training_lines_carry_a_roofline():
    """... and the training modes emit `roofline` (VERDICT r05 "next" #3b: it was `{}`): live forward + backward FLOPs against the pipe"""
    r = _run(["--train", "--steps", "3", "--warmup", "1", "--depths", "2,2"], {"IAF_BENCH_FORCE_DIST": "0"})
    assert r.returncode == 0, r.stderr[-2000:]
    rf = json.loads(r.stdout.strip().splitlines()[-1])["roofline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and rf["achieved"] > 0
    assert rf["live_gflop_per_step"]["forward"] == pytest.approx(rf["live_gflop_per_step"]["weight_gradients"])


@pytest.mark.parametrize("nht", [4, 8, 10, 12])
def test_skipped_blocks_of_the_issued_over_live_figure_are_dead_in_the_mask(nht):
    """bench.py's `roofline.issued_over_live` subtracts the centre-tap blocks a channel-triangular hidden layer of the
    one-launch step skips (`_tri_skipped`, restating iaf_step_fused.hpp's compile-time `tri_live`): every (input pair of 32
    channels, co tile of 16) block it counts must be ALL ZERO in the reference's mask (get_linear_ar_mask, layers.py:115-124,
    n_in = n_out), and at n_h = 160 that is every dead block there is"""
    import importlib.util
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from iaf_amd.layers import get_linear_ar_mask
    n = 16 * nht
    npair = -(-n // 32)
    mask = get_linear_ar_mask(n, n, zerodiagonal=False)              # [n_in, n_out]
    dead = sum(1 for c in range(npair) for t in range(nht) if not mask[32 * c:32 * c + 32, 16 * t:16 * t + 16].any())
    assert dead == sum(max(0, npair - 1 - t // 2) for t in range(nht))     # block (c, t) is dead iff c > t // 2
    skipped = bench._tri_skipped(nht, npair)
    assert 0 <= skipped <= dead and (skipped > 0 or nht == 4)      # (n_h = 64: both pairs are live for some tile of the only slot)
    if nht == 10:
        assert skipped == dead == 20


def test_profile_json_matches_the_csv_it_cites():
    """`roofline.rocprof` of the bench line reads profiles/rocprof_dominant_kernel.json, which cites a rocprofv3
    --stats CSV under profiles/rNN/ -- the average it carries must BE that CSV's row (tools/adopt_profiles.py copies both from one
    refresh), and the per-round copy beside the CSV must be the same file."""
    import csv
    import re
    top = os.path.join(ROOT, "profiles", "rocprof_dominant_kernel.json")
    j = json.load(open(top))
    m = re.match(r"(profiles/(r\d+)/bench_kernel_stats\.csv)", j["source"])
    assert m, j["source"]
    rows = [r for r in csv.DictReader(open(os.path.join(ROOT, m.group(1)))) if r["Name"] == j["kernel"]]
    assert len(rows) == 1
    assert int(rows[0]["Calls"]) == j["calls"]
    assert abs(float(rows[0]["AverageNs"]) / 1e3 - j["avg_launch_us"]) < 1e-6
    assert json.load(open(os.path.join(ROOT, "profiles", m.group(2), "rocprof_dominant_kernel.json"))) == j
    pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_dominant_kernel.json")))
    rp = re.search(r"profiles/(r\d+)/pmc/", pj["command"])
    assert rp and json.load(open(os.path.join(ROOT, "profiles", rp.group(1), "pmc_dominant_kernel.json"))) == pj


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_every_layer_and_samples_beyond_the_budget(tmp_path, monkeypatch):
    """CPU: --dump-outputs stacks each latent level's (z_new, logsd) into float32 .npy files; past the byte budget every array keeps
    the same share of its elements at the same seeded positions, so two runs with the same arguments compare element for element"""
    import numpy as np
    bench = _bench_module()
    g = torch.Generator().manual_seed(0)
    layers = [dict(H=H, out=(torch.randn(3, 4, H, H, generator=g), torch.randn(3, 4, H, H, generator=g))) for H in (16, 16, 8)]
    bench.dump_outputs(str(tmp_path / "full"), layers)
    for name, i, lv in (("z_new", 0, layers[:2]), ("logsd", 1, layers[:2]), ("z_new", 0, layers[2:]), ("logsd", 1, layers[2:])):
        H = lv[0]["H"]
        a = np.load(str(tmp_path / "full" / ("%s_%dx%d.npy" % (name, H, H))))
        assert a.dtype == np.float32 and a.shape == (len(lv), 3, 4, H, H)
        assert np.array_equal(a, torch.stack([L["out"][i] for L in lv]).numpy())
    assert sorted(os.listdir(str(tmp_path / "full"))) == ["logsd_16x16.npy", "logsd_8x8.npy", "z_new_16x16.npy", "z_new_8x8.npy"]
    total = sum(os.path.getsize(str(tmp_path / "full" / f)) for f in os.listdir(str(tmp_path / "full")))
    monkeypatch.setattr(bench, "DUMP_BYTES", total // 4)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), layers)
    for f in os.listdir(str(tmp_path / "full")):
        full, a, b = (np.load(str(tmp_path / d / f)) for d in ("full", "a", "b"))
        assert a.ndim == 1 and 0 < a.size < full.size // 3 and np.array_equal(a, b)
        assert np.isin(a, full.reshape(-1)).all()
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= total // 4 + 4 * 128


def test_steps_below_one_and_dump_outputs_outside_the_default_mode_are_refused(tmp_path):
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr and not r.stdout.strip()
    r = _run(["--train", "--dump-outputs", str(tmp_path)])
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not os.listdir(str(tmp_path))


@pytest.mark.gpu
def test_dump_outputs_hold_what_the_timed_step_computed(tmp_path):
    """--dump-outputs DIR: after the timed steps, every layer's z_new and logsd as the caller of the step receives them; the first
    16x16 layer (bench.py's seeded inputs) against the CPU oracle"""
    import numpy as np
    from oracle import iaf_oracle as O
    bench = _bench_module()
    r = _run(["--steps", "3", "--warmup", "1", "--repeats", "1", "--settle-seconds", "0", "--depths", "2,2", "--no-cpu-baseline",
              "--no-modes", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    got = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert sorted(got) == ["logsd_16x16", "logsd_8x8", "z_new_16x16", "z_new_8x8"]
    for k, a in got.items():
        H = int(k.split("_")[-1].split("x")[0])
        assert a.dtype == np.float32 and a.shape == (2, 32, 32, H, H) and np.isfinite(a).all(), k
    params, z, ctx = bench.make_layer_inputs(np.random.RandomState(1234), 32, 32, 160, 2, 16)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    ez, es = O.iaf_step(f32(z), f32(ctx), {k: f32(v) for k, v in params.items()}, [160, 160])
    assert np.abs(got["z_new_16x16"][0] - ez).max() < 1e-4 and np.abs(got["logsd_16x16"][0] - es).max() < 1e-4
