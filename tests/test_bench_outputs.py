"""bench.py's plain run and --dump-outputs: the files hold what the last timed step computed, in float32 / float64, bits past a row's
length cleared, long arrays sampled at fixed positions; on the GPU the dumped step equals the CPU oracle's rows for the GOP it coded."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_for_output_tests", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rows():
    """Two coded rows with garbage past their lengths (n = 13 pixels: 2 mask bytes) and one pair across a keyframe."""
    return [{"mask": np.array([0xFF, 0xFF], np.uint8), "ones": 13, "k": 2.25, "l": 10, "filter": np.array([0xAB, 0xFF], np.uint8),
             "witness": np.array([0xF0], np.uint8), "witness_bits": 3},
            {"skipped": True, "mask": np.zeros(2, np.uint8), "ones": 0, "k": 0.0, "l": 0, "witness_bits": 0},
            {"mask": np.array([0x80, 0x0F], np.uint8), "ones": 1, "k": 1.5, "l": 0, "filter": np.zeros(0, np.uint8),
             "witness": np.zeros(0, np.uint8), "witness_bits": 0}]


def test_dump_outputs_layout(tmp_path):
    bench = _load_bench()
    bench.dump_outputs(str(tmp_path), _rows(), 13)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["filter", "k", "l", "mask", "ones", "skipped", "witness", "witness_bits"]
    for name in ("k", "l", "ones", "witness_bits", "skipped"):
        assert got[name].dtype == np.float64 and got[name].shape == (3,)
    assert got["k"].tolist() == [2.25, 0.0, 1.5] and got["l"].tolist() == [10, 0, 0] and got["skipped"].tolist() == [0, 1, 0]
    assert got["mask"].dtype == got["filter"].dtype == got["witness"].dtype == np.float32
    assert got["mask"].tolist() == [0xFF, 0xF8, 0, 0, 0x80, 0x08]        # 13 bits per row
    assert got["filter"].tolist() == [0xAB, 0xC0] and got["witness"].tolist() == [0xE0]


def test_dump_outputs_samples_long_arrays_at_fixed_positions(tmp_path, monkeypatch):
    bench = _load_bench()
    monkeypatch.setitem(bench.DUMP_MAX_VALUES, "mask", 4)
    rows = [dict(_rows()[0], mask=np.arange(8, dtype=np.uint8)) for _ in range(2)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rows, 64)
    a, b = np.load(tmp_path / "a" / "mask.npy"), np.load(tmp_path / "b" / "mask.npy")
    assert a.shape == (4,) and np.array_equal(a, b)
    assert set(a.tolist()) <= set(range(8))


def test_dump_outputs_refused_in_clip_mode(tmp_path):
    """--dump-outputs names the GOP pipelines' last step; the clip mode has none: the run says so (failure line, exit 1) before any device work."""
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--clip-frames", "21", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 1
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["value"] is None and "--dump-outputs" in line["error"]
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path, oracle):
    """A plain run: the contract's keys, exactly --steps timed steps, none of --full's measurements; the dump is the last timed step's
    rows, equal to the CPU oracle's for the GOP that step coded."""
    from new_bloom_filter_repo_amd.synthetic import make_gop
    from test_gpu_bench_shape import oracle_gop
    W, H, F, steps, warmup = 640, 360, 8, 5, 2
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "bench.py", "--steps", str(steps), "--warmup", str(warmup), "--width", str(W), "--height", str(H),
                        "--frames", str(F), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == steps and res["warmup"] == warmup and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["unit"] == "Mpixel/s" and res["higher_is_better"] is True and res["dtype"] == "u64"
    assert abs(res["value"] - res["config"]["pixels_per_step"] / (res["ms_per_step"] * 1e3)) <= 0.01 * res["value"]
    for key in ("verified_vs_oracle", "cpu_baseline", "roofline", "steady_state", "clip300", "decode_1080p"):
        assert key not in res, key
    # step s codes pipeline s % 4's resident GOP (s // 4) % 3; bench_main seeds it 2000 + k + 16 g (rank 0, one GOP per call)
    s = warmup + steps - 1
    k, g = s % 4, (s // 4) % 3
    want = oracle_gop(oracle, np.stack(make_gop(2000 + k + 16 * g, W, H, F)))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    n = W * H
    masks = got["mask"].astype(np.uint8).reshape(F - 1, n // 8)
    fo = wo = 0
    for f, (mask, ones, kk, l, bit_array, witness) in enumerate(want):
        assert np.array_equal(np.unpackbits(masks[f]), mask) and got["ones"][f] == ones, f
        assert (got["k"][f], got["l"][f]) == (kk, l), f
        if not l:
            continue
        fb, wb = (l + 7) // 8, (len(witness) + 7) // 8
        assert np.array_equal(got["filter"][fo:fo + fb].astype(np.uint8), np.packbits(bit_array)), f
        assert got["witness_bits"][f] == len(witness) and np.array_equal(got["witness"][wo:wo + wb].astype(np.uint8), np.packbits(witness)), f
        fo, wo = fo + fb, wo + wb
    assert fo == got["filter"].size and wo == got["witness"].size
