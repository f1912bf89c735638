"""CPU: bench.py's N > 1 rank logic, executed (VERDICT r2 item 8 -- no multi-GPU node was available to the driver in rounds 1-2, so the branch the
first real 8-GPU run takes had never run anywhere).  `bench.py --gpus 2 --dry-run-emu` re-executes itself under torch.distributed.run exactly as
`--gpus 2` does on a GPU box, every rank reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*, installs the CPU emulator instead of a HIP device and
gloo instead of RCCL, and runs the shared code of main(): K timed steps between fences (barrier), max over ranks (all_reduce MAX), the DDP
training probe (`smart_DDP`: parameter broadcast, loss * WORLD_SIZE as train.py:404-405, bucketed all-reduce(mean) of the flat gradient arena
overlapped with the backward plan), rank 0 printing ONE JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_bench_two_rank_dry_run_on_the_emulator():
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None), env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-emu", "--model", "yolov5n", "--batch", "2", "--imgsz", "64",
           "--steps", "2", "--warmup", "1"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=850)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]          # rank 0 only, one line
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in r, k
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["warmup"] == 1 and r["scaling"] == "weak" and r["higher_is_better"] is True
    assert r["config"]["global_batch"] == 4 and r["value"] > 0
    assert abs(r["value"] - 4 * 2 / (r["ms_per_step"] * 2 * 1e-3)) < 0.02 * r["value"]     # whole-job images / max-over-ranks time
    t = r["train"]
    assert t["rccl_ranks"] == 2 and t["allreduce_buckets"] >= 1
    # the all-reduced bytes are the flat fp32 gradient arena: every parameter in a 64-float padded slot (yolov5n: 7.49 MB; yolov5s: 28.94 MB)
    sys.path.insert(0, ROOT)
    from yolov5_amd.yolo import DetectionModel

    want = sum(-(-p_.numel() // 64) * 64 * 4 for p_ in DetectionModel("yolov5n.yaml").parameters())
    assert t["allreduce_bytes_per_step"] == want, (t["allreduce_bytes_per_step"], want)
    assert t["loss"] > 0 and t["images_per_sec"] > 0


@pytest.mark.timeout(900)
def test_bench_dump_outputs_repeat_identically(tmp_path):
    """--dump-outputs: after the timed steps (exactly --steps of them) the per-image detections of the last one land in DIR as float32 .npy files;
    two runs with the same arguments see the same inputs and write the same arrays."""
    import numpy as np

    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None), env.pop("LOCAL_RANK", None)
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run-emu", "--model", "yolov5n", "--batch", "2", "--imgsz", "64",
               "--steps", "3", "--warmup", "1", "--no-train", "--dump-outputs", str(d)]
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        r = json.loads(lines[0])
        assert r["steps"] == 3 and r["step_ms"]["n"] == 3     # one step time per timed step
        assert r["ms_per_step"] > 0 and abs(r["value"] - 2 * 3 / (r["ms_per_step"] * 3 * 1e-3)) < 0.02 * r["value"]
        files = sorted(os.listdir(d))
        assert files == ["det_0000.npy", "det_0001.npy"], files
        arrs = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 6 for a in arrs.values())
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_bench_op_table_needs_full(tmp_path):
    """The per-op table is a --full measurement: asked for on a plain run, bench.py refuses before any work instead of quietly skipping it."""
    out = tmp_path / "ops.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--op-table", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--op-table needs --full" in p.stderr, (p.returncode, p.stderr[-2000:])
    assert not out.exists()
