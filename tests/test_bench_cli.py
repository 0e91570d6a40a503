"""bench.py's command line: a plain run prints the headline line alone (what takes runs of its own sits
behind --full), and --dump-outputs writes the textures of the last timed step, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "kernels_us", "ifft_stage", "cache", "update_loop", "cpu_baseline")


def run_bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=300, check=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def load_dir(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_cfg1_dump_outputs_repeat(tmp_path):
    """The CPU-only line (cfg1) with --dump-outputs: float32 DISP, DERIV and TURB of the last timed frame,
    bit-identical between two runs with the same arguments."""
    pytest.importorskip("torch")
    dumps = []
    for k in range(2):
        d = run_bench("--config", "cfg1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"d{k}"))
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        dumps.append(load_dir(tmp_path / f"d{k}"))
    assert sorted(dumps[0]) == ["deriv.npy", "disp.npy", "turb.npy"]
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and a.shape == (1, 256, 256, 4) and np.isfinite(a).all() and np.abs(a).max() > 0
        np.testing.assert_array_equal(a, dumps[1][name])


@pytest.mark.gpu
def test_full_run_keeps_the_kernel_figures(require_gpu):
    """--full prints the headline keys and the fields the A/B and profiling tools read (kernels_us, roofline);
    the long legs are switched off here by their own options, as those tools do."""
    d = run_bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-ifft-stage",
                  "--no-beyond-cache", "--no-update-loop")
    for k in HEADLINE + FULL_ONLY:
        assert k in d, k
    assert set(d["kernels_us"]) == {"pass_a", "pass_b"} and min(d["kernels_us"].values()) > 0
    assert d["roofline"]["kernel"] in ("pass_a", "pass_b") and d["roofline"]["frac"] > 0
    assert d["frame"]["ms_per_step_with_kernel_events"] > 0


@pytest.mark.gpu
def test_plain_run_line_and_dump(require_gpu, tmp_path):
    """A plain cfg3 run: one JSON line with the headline keys and none of --full's measurements,
    ms_per_step consistent with value over the K timed steps, and a dump of at most 64 MB whose
    elements are those of the same frames stepped through the binding here (W + K steps from zero
    foam on the same seeded noise), at the sample bench.write_outputs documents."""
    sys.path.insert(0, ROOT)
    import bench
    import ocean_hip as oh
    from ocean_hip.shard import tile_seed
    W, K = 2, 3
    d = run_bench("--gpus", "1", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "d"))
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == K and d["warmup"] == W and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-3)  # one ocean per step at cfg3
    got = load_dir(tmp_path / "d")
    assert sorted(got) == ["deriv.npy", "disp.npy", "turb.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64e6

    n, C = 1024, 4
    size = C * n * n * 4
    keep = bench.DUMP_BUDGET_BYTES // 4 // 3
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, size, keep))
    with oh.OceanContext(n, C, 1, 0) as ctx:
        ctx.set_params(bench.SCENE_PARAMS, bench.SCENE_CASCADES)
        ctx.generate_noise(tile_seed(20251121, 0))
        ctx.init_spectrum()
        for f in range(W + K):
            ctx.step(f / 60.0)
        ctx.synchronize()
        for name, tex in (("disp", oh.TEX_DISP), ("deriv", oh.TEX_DERIV), ("turb", oh.TEX_TURB)):
            a = got[name + ".npy"]
            assert a.dtype == np.float32 and a.shape == (keep,)
            np.testing.assert_array_equal(a, ctx.read_all(tex).reshape(-1)[idx], err_msg=name)
