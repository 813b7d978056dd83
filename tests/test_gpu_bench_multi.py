"""bench.py's N > 1 branch on ONE GPU: two ranks under torch.distributed.run share GPU 0, the frame-closing gather runs
over gloo through host staging (EZRT_BENCH_BACKEND=gloo) but through the SAME code path as the driver's RCCL runs --
tile sharding inside the kernels, the library's pack / un-permute kernels, the timed windows, MAX over ranks, the
1-GPU reference frame and the C4 strong-scaling variant.  So that the first run on an 8-GPU node does not die of a typo
(VERDICT r2 #6)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(scaling, port, ranks=2, spp=8):
    env = dict(os.environ, EZRT_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(ranks), "--steps", "2", "--warmup", "1", "--windows", "3",
           "--spp", str(spp), "--cpu-seconds", "0"] + (["--scaling", scaling] if scaling else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # rank 0 prints ONE JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("scaling,port", [("weak", 29631), ("strong", 29633)])
def test_bench_two_ranks_on_one_gpu(scaling, port):
    out = _run(scaling, port)
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["steps"] == 2 and out["warmup"] == 1
    assert out["unit"] == "Mrays/s" and out["value"] > 0 and out["ms_per_step"] > 0
    t = out["timing"]
    assert len(t["window_ms"]) == 3 and min(t["window_ms"]) > 0
    assert abs(out["ms_per_step"] * 2 - sorted(t["window_ms"])[1]) < 1e-2      # value comes from the MEDIAN window
    spp = 16 if scaling == "weak" else 8
    assert "%d spp" % spp in out["config"]["workload"]
    mg = out["multi_gpu"]
    assert mg["tiles_total"] == 32 * 32 and mg["tiles_per_rank"] == [512, 512]
    assert all(x > 0 for x in mg["render_ms_per_rank_median"])
    one = mg["one_gpu_same_frame"]
    assert one["bit_identical_to_n_gpu_frame"] is True and one["linf_vs_n_gpu_frame"] == 0.0
    assert one["Mrays_s"] > 0
    c4 = mg["c4_strong_variant"]
    assert c4["Mrays_s"] > 0 and c4["one_gpu_same_frame"]["bit_identical_to_n_gpu_frame"] is True
    if scaling == "strong":   # (round 4: the weak run is an extra field of the strong line)
        w = mg["weak_variant"]
        assert w["scaling"] == "weak" and w["Mrays_s"] > 0 and "16 spp" in w["workload"]
    else:
        assert "weak_variant" not in mg


def test_bench_eight_ranks_on_one_gpu_default_is_strong():
    """The driver's N = 8 command line (no --scaling flag) with all eight ranks on GPU 0 over gloo: the default is the STRONG
    split of the fixed frame, 128 tiles per rank, the frame bit-identical to the 1-GPU frame."""
    out = _run(None, 29641, ranks=8, spp=4)
    assert out["n_gpus"] == 8 and out["scaling"] == "strong"
    assert "4 spp" in out["config"]["workload"]
    mg = out["multi_gpu"]
    assert mg["tiles_per_rank"] == [128] * 8 and len(mg["render_ms_per_rank_median"]) == 8
    assert mg["one_gpu_same_frame"]["bit_identical_to_n_gpu_frame"] is True
    assert mg["c4_strong_variant"]["one_gpu_same_frame"]["bit_identical_to_n_gpu_frame"] is True
    assert mg["weak_variant"]["Mrays_s"] > 0


def test_bench_single_gpu_line_carries_parity_configs_and_model():
    """The N = 1 line at reduced sizes (the driver's run uses the defaults): the timed frame equals the instrumented route's
    frame and the CPU oracle's; C3 / C4 / C5 are timed with a crop of the timed frame equal to the oracle's; the scaling
    model has C2 and C4 for 2 / 4 / 8 shards; both VALU peaks are printed; the reference's compiled shader is timed."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--windows", "3", "--spp", "3",
           "--config-spp", "2", "--cpu-seconds", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["scaling"] == "n/a" and out["value"] > 0
    par = out["parity"]
    assert par["timed_frame_equals_instrumented_frame"] is True and par["rays_timed_route_equals_instrumented_route"] is True
    assert out["cpu_baseline"]["linf_vs_gpu"] == 0.0 and out["cpu_baseline"]["kind"] == "port"
    ref = out["cpu_baseline"]["reference_shader"]
    assert ref["port_frame_equals_reference_shader_frame"] is True and out["cpu_baseline"]["reference_shader_one_thread_Mrays_s"] > 0
    for nm in ("C3", "C4", "C5"):
        c = out["configs"][nm]
        assert "error" not in c, c
        assert c["Mrays_s"] > 0 and c["rays"] > 0 and c["trace_ms"] > 0
        assert c["crop_vs_oracle"]["bit_identical"] is True and c["crop_vs_oracle"]["crop_max"] > 0.05
    rf = out["roofline"]
    # (the measured ceiling is read from the round's microbenchmark log, profiles/r5/valu_issue_microbench.txt; 1.086 is the fall-back)
    assert 0.9 < rf["peak_measured"] < 1.2 and abs(rf["peak_nominal"] - 1.2288) < 1e-3
    assert out["value_lone_call"] > 0 and out["ms_per_step_lone_call"] > 0   # the un-pipelined rate beside the headline (VERDICT r4 #5c)
    for k in ("C2", "C4"):
        sh = out["scaling_model"][k]["shards"]
        assert set(sh) == {"2", "4", "8"} and all(v["predicted_speedup"] > 0 for v in sh.values())
        assert len(sh["8"]["render_ms_per_shard"]) == 8


def test_bench_plain_run_is_the_headline_alone_and_dumps_the_timed_frame(tmp_path, oracle):
    """A plain run (no --full) times exactly --steps steps in one window, prints the headline fields and nothing that needs
    runs of its own, and --dump-outputs writes the frame the last timed step left: on the bits the CPU oracle's frame."""
    import numpy as np
    from ezrt_amd import scene as S, scenes, trace
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--width", "64", "--height", "64",
           "--spp", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["value"] > 0
    assert out["steps"] == 3 and len(out["timing"]["window_ms"]) == 1
    assert abs(out["ms_per_step"] * 3 - out["timing"]["window_ms"][0]) < 1e-2
    for k in ("parity", "roofline", "configs", "cpu_baseline", "scaling_model", "value_lone_call", "multi_gpu"):
        assert k not in out, k
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (64, 64, 4)
    cfg = scenes.CONFIGS["C2"]
    bs = scenes.bunny_scene(subdiv=2, want_cache=False, hdr="shipped")
    eye, cam = S.camera(*cfg["camera"])
    so = bs.upload(oracle)
    want = so.render(trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2))
    so.close()
    ua, ub = got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert ((ua == ub) | (np.isnan(got) & np.isnan(want))).all()
