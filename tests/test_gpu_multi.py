"""The multi-GPU code paths on the one-GPU box: RCCL (backend nccl) with a one-rank group, bench.py's own rank spawning, and
the bench line's contract fields.  N > 1 ranks on separate GPUs are the driver's to run (SCALE); these tests make sure that what
it will launch has executed before: process-group setup with device_id, all-gather / all-reduce / barrier on GPU tensors through
RCCL, shard.make_ba_exchange's nccl branch, and `bench.py --gpus N` starting N ranks by itself."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_NCCL_WORKER = r"""
import os, sys
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import numpy as np, torch, torch.distributed as dist
import orbhip, shard
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
# shard.make_ba_exchange, nccl branch: slot `rank` of the exchange buffer all-gathered in place through RCCL
stride = 1000
xbuf = torch.zeros(stride, dtype=torch.float64, device="cuda")
xbuf[:600] = torch.arange(600, dtype=torch.float64, device="cuda") * 0.5
ex = shard.make_ba_exchange(xbuf, stride)
ex(2, 600)
assert torch.equal(xbuf[:600].cpu(), torch.arange(600, dtype=torch.float64) * 0.5) and float(xbuf[600:].abs().sum()) == 0.0
# the ORB path's only exchange: fixed-size per-frame records, and the max over ranks of the timed region
rec = torch.arange(24, dtype=torch.int32, device="cuda").view(12, 2)
allrec = shard.allgather_records(rec)
assert tuple(allrec.shape) == (1, 12, 2) and torch.equal(allrec[0], rec)
assert shard.max_over_ranks(3.25, device="cuda") == 3.25
dist.barrier()
# a real extraction next to the live process group (one HIP runtime serves torch, RCCL and liborbhip)
ctx = orbhip.Context(0); ext = orbhip.Extractor(ctx, 500, 1.2, 8, 20, 7)
r = ext.extract_host(orbhip.synth_frames(320, 240, 2, seed=3), (0, 0))
assert len(r[0][0]) > 300
ext.close(); ctx.close()
dist.destroy_process_group()
print("NCCL_OK")
"""


def _env(**kw):
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    e.update(kw)
    return e


def test_one_rank_nccl_group_runs_the_rccl_paths(tmp_path):
    script = tmp_path / "w.py"
    script.write_text("ROOT = %r\n" % ROOT + _NCCL_WORKER)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                        "--master-port", "29641", str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=_env(), timeout=400)
    assert r.returncode == 0 and "NCCL_OK" in r.stdout, r.stdout[-3000:]


SMALL = ["--full", "--steps", "2", "--warmup", "1", "--batch", "32", "--ba-graphs", "4", "--ba-steps", "1", "--pose-frames", "32",
         "--stereo-pairs", "8", "--no-cpu-baseline"]


def _line(stdout):
    lines = [l for l in stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-3000:]
    return json.loads(lines[0])


def test_bench_one_rank_over_rccl():
    """bench.py with the process group forced on for one rank: init_process_group("nccl", device_id=...), the rank census, barriers,
    max-over-ranks and the record all-gather all run through RCCL on this box's GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=_env(ORBHIP_BENCH_FORCE_DIST="1"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 1 and d["config"]["ranks_seen"] == [0] and d["config"]["collective_backend"] == "nccl"
    assert d["config"]["records_gathered"] == 32 and d["value"] > 0 and d["ba"]["value"] > 0
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"]
    assert d["roofline"]["kernel"].startswith("k_") and 0 < d["roofline"]["frac"] < 1


def test_bench_gpus2_spawns_two_ranks_itself():
    """`python bench.py --gpus 2` with no torch.distributed environment must start two ranks by itself (the driver's SCALE command
    shape).  Rehearsal on one card: both ranks pinned to GPU 0, collectives over gloo; the line must say n_gpus 2, list both ranks
    and count both ranks' records."""
    env = _env(ORBHIP_BENCH_BACKEND="gloo", ORBHIP_BENCH_DEVICE="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--ba-sharded-graphs", "2"] + SMALL,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["ranks_seen"] == [0, 1] and d["config"]["frames_total"] == 64
    assert d["config"]["records_gathered"] == 64 and d["scaling"] == "weak"
    assert "error" not in d["ba_sharded"] and d["ba_sharded"]["ranks"] == 2 and d["ba_sharded"]["all_gathers"] > 3
    assert "cpu_baseline" not in d


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py` run prints the headline line alone (the profiled pass and the other legs are `--full`'s), and
    `--dump-outputs DIR` writes what its last timed step computed: checked here against the CPU oracle on the same frames."""
    import numpy as np
    import orbhip
    import oracle_bind as ob
    import oracle_match_bind as om
    out = tmp_path / "dump"
    B = 32
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("ORB extract+match frames/sec", "frames/s", True, "u8")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - B * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    for k in ("roofline", "ba", "pose_opt", "stereo", "tracking", "inertial_ba", "hd", "4k", "latency", "cpu_baseline"):
        assert k not in d, k
    files = sorted(out.iterdir())
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    a = {f.name[:-4]: np.load(f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    cnt = a["keypoint_counts"].astype(np.int64)
    frames = a["sampled_frames"].astype(np.int64)
    assert len(cnt) == B and (cnt > 0).all() and list(frames) == list(range(B))       # a batch this small is sampled whole
    imgs = orbhip.synth_frames(640, 480, B, seed=20241004)                             # the bench's frames
    ora = ob.OracleExtractor(1000, 1.2, 8, 20, 7)
    res = [ora.extract(imgs[f], (0, 0)) for f in range(B)]
    assert list(cnt) == [len(kp) for kp, _, _ in res]
    kp = np.concatenate([kp for kp, _, _ in res])
    np.testing.assert_array_equal(a["keypoints"], np.stack([kp[n].astype(np.float32) for n in kp.dtype.names], 1))
    np.testing.assert_array_equal(a["descriptors"], np.concatenate([ds for _, ds, _ in res]).astype(np.float32))
    bf = [om.bf2nn(res[f][1], res[(f + 1) % B][1], 0.7) for f in range(B)]
    np.testing.assert_array_equal(a["bf2nn_index"], np.concatenate([x[0] for x in bf]))
    np.testing.assert_array_equal(a["bf2nn_distance"], np.concatenate([x[1] for x in bf]))
    np.testing.assert_array_equal(a["bf2nn_accept"], np.concatenate([x[2] for x in bf]))
    si = [om.search_for_initialization(res[f][0], res[f][1], res[f + 1][0], res[f + 1][1], (0.0, 0.0, 640.0, 480.0),
                                       np.stack([res[f][0]["x"], res[f][0]["y"]], 1), 100, 0.9, True) for f in range(B - 1)]
    np.testing.assert_array_equal(a["search_init_nmatches"], [x[0] for x in si])
    np.testing.assert_array_equal(a["search_init_matches12"], np.concatenate([x[1] for x in si]))
    np.testing.assert_array_equal(a["search_init_prev_matched"], np.concatenate([x[2] for x in si]))
