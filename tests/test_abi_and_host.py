"""CPU tests: the C-ABI library loads and exports every symbol include/orbhip.h declares; host-side
helpers; the product refuses to run without a device (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(orbhip_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    import orbhip
    syms = _declared_symbols()
    assert len(syms) >= 131 and "orbhip_extractor_fast_kernel" in syms and "orbhip_extractor_blur_kernel" in syms
    missing = [s for s in syms if not hasattr(orbhip.lib, s)]
    assert not missing, missing
    assert orbhip.lib.orbhip_version().startswith(b"orbhip")


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "orbhip.h"\nint main(void){orbhip_keypoint k; (void)k; return sizeof(orbhip_keypoint)==28?0:1;}\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        assert subprocess.call([str(exe)]) == 0


def test_no_device_no_fallback():
    """On a box without a GPU the product must fail loudly (ORBHIP_E_NODEVICE), never compute on the CPU."""
    import orbhip
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.Context(0)
    assert ei.value.code == orbhip.E_NODEVICE


def test_product_does_not_reference_oracle():
    """The product tree must never import / link / load anything under oracle/."""
    pkg = os.path.join(ROOT, "orb-slam3-mac_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".hip", ".h", ".c", ".cc", ".cpp", ".py", "Makefile")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "oracle_bind" not in txt and "liborb_oracle" not in txt and "orc_" not in txt, os.path.join(dp, fn)
    out = subprocess.run(["ldd", os.path.join(pkg, "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    assert "oracle" not in out


def test_host_descriptor_distance_is_pure_host():
    import orbhip
    a = np.arange(32, dtype=np.uint8)
    b = a[::-1].copy()
    assert orbhip.descriptor_distance(a, b) == int(np.unpackbits(a ^ b).sum())


def test_synth_generator_deterministic_and_textured():
    import orbhip
    a = orbhip.synth_frames(160, 120, 3, seed=5)
    b = orbhip.synth_frames(160, 120, 3, seed=5)
    c = orbhip.synth_frames(160, 120, 1, seed=5, first=2)
    assert (a == b).all() and (a[2] == c[0]).all() and not (a[0] == a[1]).all()
    assert a.std() > 20


def test_frame_range_partition():
    import shard
    for total, world in [(1024, 8), (10, 3), (5, 8), (4096, 8)]:
        spans = [shard.frame_range(r, world, total) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1


_WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import shard, orbhip, oracle_bind as ob
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
TOTAL, W, H = 6, 160, 120
lo, hi = shard.frame_range(rank, world, TOTAL)
# stand-in for the per-rank HIP extraction (no GPU in CI): the shard logic and the collective are what is tested
imgs = orbhip.synth_frames(W, H, hi - lo, seed=99, first=lo)
e = ob.OracleExtractor(200, 1.2, 4, 20, 7)
rec = torch.zeros((3, 2), dtype=torch.int32)
for i in range(hi - lo):
    kp, desc, mono = e.extract(imgs[i], (0, 0))
    rec[i, 0] = len(kp); rec[i, 1] = mono
allrec = shard.allgather_records(rec)
tmax = shard.max_over_ranks(1.0 + rank)
if rank == 0:
    full = orbhip.synth_frames(W, H, TOTAL, seed=99)
    want = []
    for i in range(TOTAL):
        kp, desc, mono = e.extract(full[i], (0, 0))
        want.append((len(kp), mono))
    got = []
    for r in range(world):
        a, b = shard.frame_range(r, world, TOTAL)
        got += [tuple(int(v) for v in allrec[r, i]) for i in range(b - a)]
    assert got == want, (got, want)
    assert tmax == float(world)
    print("GLOO_OK")
dist.destroy_process_group()
'''


def test_two_rank_gloo_shard_and_gather(tmp_path):
    """world_size 2 over gloo: contiguous frame shards, one all-gather of fixed-size records, max-over-ranks."""
    script = tmp_path / "w.py"
    script.write_text("ROOT = %r\n" % ROOT + _WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29611")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29611", str(script)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "GLOO_OK" in r.stdout, r.stdout[-3000:]


def test_bench_spawns_ranks_before_touching_the_gpu(monkeypatch):
    """`bench.py --gpus N` outside a torch.distributed environment: N ranks are started as a child `torch.distributed.run`, from a
    process that has imported neither torch nor the HIP library (a process that has initialised the GPU must never re-launch)."""
    import importlib
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--workload", "hd"])
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        seen["torch_loaded"] = "torch" in sys.modules and getattr(sys.modules["torch"], "cuda", None) is not None and sys.modules["torch"].cuda.is_initialized()
        seen["orbhip_loaded"] = "orbhip" in sys.modules
        return 7
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    was_orbhip = "orbhip" in sys.modules
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 7                                  # the child's return code is passed through
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "3", "--workload", "hd"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and not seen["torch_loaded"]
    assert seen["orbhip_loaded"] == was_orbhip                 # spawning itself loads nothing
    # inside a launcher's environment nothing is spawned; a mismatching --gpus is refused loudly
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert "WORLD_SIZE" in str(ex.value.code)


def test_bench_workloads_match_baseline_configs():
    import importlib
    bench = importlib.import_module("bench")
    a = bench.parse_args([])
    assert (a.workload, a.width, a.height, a.nfeatures, a.batch, a.gpus) == ("vga", 640, 480, 1000, 1024, 1)      # configs[1]
    a = bench.parse_args(["--workload", "hd", "--gpus", "8"])
    assert (a.width, a.height, a.nfeatures, a.batch * a.gpus) == (1920, 1080, 2000, 4096)                         # configs[2]
    ab = bench.algorithmic_bytes(640, 480, 1000, 0)
    assert ab["S"] == 950532 and ab["total"] == 5742474


def test_bench_plain_run_is_the_default():
    """Without --full a run is the headline step alone; --full and --dump-outputs are opt-in."""
    import importlib
    bench = importlib.import_module("bench")
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert (a.full, a.dump_outputs) == (True, "out")


def test_reference_call_lines_compile_against_the_host_classes(tmp_path):
    """The drop-in claim, compile-only: host/compile_callers.cc holds the call lines of the reference's Tracking (src/Tracking.cc:1505-1506,
    1757-1775, 1881-1934, 1996-2002, 2405-2428, 2645-2753), LocalMapping (src/LocalMapping.cc:138-154, 407-463, 781-817), LoopClosing
    (src/LoopClosing.cc:578-755, 1005-1008, 1722, 2284-2340) and Frame::ExtractORB (src/Frame.cc:410-417) as the reference writes them; it must
    build against host/ORBextractor.h, host/ORBmatcher.h and host/Optimizer.h with -Wall -Werror, and every class method it calls must be
    DEFINED by the host sources (a link of the same unit against them resolves)."""
    import subprocess
    host = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
    obj = str(tmp_path / "callers.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(host, "compile_callers.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::ORBmatcher::" in ln or "ORB_SLAM3::Optimizer::" in ln or "ORB_SLAM3::ORBextractor::" in ln]
    assert len(wanted) >= 18, wanted                           # 13 matcher methods + ctor, 4 optimiser entry points, the extractor's operator()
    defined = ""
    for src in ("ORBmatcher.cc", "ORBmatcher_keyframe.cc", "Optimizer_LocalBA.cc", "Optimizer_LocalInertialBA.cc", "Optimizer_PoseOptimization.cc",
                "Optimizer_MergeBA.cc", "ORBextractor.cc"):
        o = str(tmp_path / (src + ".o"))
        r = subprocess.run(["g++", "-std=c++17", "-O0", "-c", "-o", o, os.path.join(host, src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        defined += subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    missing = [w for w in wanted if w not in defined]
    assert not missing, missing


def test_every_environment_variable_the_library_reads_is_documented():
    """INTEGRATION.md section 5 lists every ORBHIP_* variable the sources read (getenv / the tune_int hook): a switch nobody can look up is
    a behaviour nobody can reproduce."""
    import glob
    import re
    names = set()
    for f in glob.glob(os.path.join(ROOT, "orb-slam3-mac_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "orb-slam3-mac_amd", "host", "*")):
        if os.path.isfile(f):
            names |= set(re.findall(r'(?:getenv|tune_int)\("(ORBHIP_[A-Z0-9_]+)"', open(f, errors="ignore").read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(names) > 20
    missing = sorted(n for n in names if n not in doc)
    assert not missing, missing
