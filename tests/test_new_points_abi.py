"""CreateNewMapPoints on the device, the parts that need no GPU: the symbols and their declarations, the Python binding, the reference's
call line against the LocalMapping stand-in, and the class without a GPU (one message, nothing created)."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")


def _nm(path, *flags):
    return subprocess.run(["nm", *flags, path], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    exported = _nm(os.path.join(PKG, "lib", "liborbhip.so"), "-D", "--defined-only")
    for name in ("orbhip_create_new_map_points_device", "orbhip_create_new_map_points_host"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert re.search(r" T %s$" % name, exported, re.M), name
    assert "typedef struct orbhip_newpoints_pair" in hdr and "typedef struct orbhip_newpoints_keyframe" in hdr


def test_binding_is_present():
    import orbhip
    import new_points_model as npm
    assert callable(orbhip.create_new_map_points_device) and callable(orbhip.create_new_map_points_host)
    assert orbhip.NEWPOINTS_PAIR_DTYPE == npm.PAIR_DTYPE
    import ctypes
    assert ctypes.sizeof(orbhip.NewPointsPair) == orbhip.NEWPOINTS_PAIR_DTYPE.itemsize
    for (name, _), field in zip(orbhip.NewPointsPair._fields_, orbhip.NEWPOINTS_PAIR_DTYPE.names):
        assert name == field and getattr(orbhip.NewPointsPair, name).offset == orbhip.NEWPOINTS_PAIR_DTYPE.fields[field][1]


def test_call_line_compiles_and_the_method_is_defined():
    r = subprocess.run(["make", "-s", "lib/compile_callers_localmapping.o", "lib/host_newpoints_smoke"], cwd=PKG, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    caller = _nm(os.path.join(PKG, "lib", "compile_callers_localmapping.o"), "-C")
    assert re.search(r" U ORB_SLAM3::LocalMapping::CreateNewMapPoints\(\)$", caller, re.M), caller
    driver = _nm(os.path.join(PKG, "lib", "host_newpoints_smoke"), "-C")
    assert re.search(r" T ORB_SLAM3::LocalMapping::CreateNewMapPoints\(\)$", driver, re.M)


def test_class_without_a_gpu_creates_nothing(tmp_path):
    import synth_new_points as sy
    from synth_sim3 import read_flat, write_flat
    arrays, used, kf_of = sy.class_case("stereo", -1)
    fin, fout = str(tmp_path / "np.in"), str(tmp_path / "np.out")
    write_flat(fin, arrays)
    r = subprocess.run([os.path.join(PKG, "lib", "host_newpoints_smoke"), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120, env=dict(os.environ, ORBHIP_DEVICE="4096"))   # no such device: the calling thread gets no context, here and on a GPU machine
    assert r.returncode == 0, r.stdout
    assert "no usable GPU" in r.stdout and "0 map points created" in r.stdout
    out = read_flat(fout)
    assert out["n_created"][0] == 0 and len(out["pos"]) == 0
    for k in range(int(arrays["nkf"][0])):
        assert np.array_equal(out["kfmp%d" % k], np.where(arrays["mp%d" % k] != 0, -2, -1))
