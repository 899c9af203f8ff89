"""CPU tests of the KeyFrameDatabase work: the two Python models (kfdb_model.py: inverted file + keyframe objects, a transcription of
src/KeyFrameDatabase.cc; kfdb_scan_model.py: arrays + the (smallest shared word, add sequence) order the device uses) agree exactly on
seeded scripts -- the premise of scanning without linked lists --, the hand-written cases give the lists the reference's text gives, wrong
rules are told from right ones, the score's summation error is bounded, the new symbols are declared, exported and bound, and the
reference's own call lines compile against the host class.  Parity everywhere is against these models, written from the reference's
text, not against a DBoW2 build."""
import math
import os
import re
import subprocess
import numpy as np
import pytest
import kfdb_cases
import kfdb_model as km
import synth_kfdb as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
CASES = kfdb_cases.cases()


@pytest.mark.parametrize("block", range(8))
def test_models_agree_on_seeded_scripts(block):
    """240 scripts of 60 operations with interleaved erase, re-add, clear_map, clear and reset: every list, every float bit pattern and all
    six state fields of every keyframe after every operation"""
    detects = outputs = readds = 0
    for seed in range(block * 30, block * 30 + 30):
        world = sk.make_world(seed, bad_maps=[2] if seed % 3 == 0 else [], vocab=40 + seed % 50)
        ops = sk.make_script(world, 60, seed=seed)
        a, b = sk.play_model(world, ops), sk.play_scan(world, ops)
        assert a[0] == b[0], seed
        assert a[1] == b[1], seed
        detects += len(a[0]); outputs += sum(len(r["loop"]) + len(r["merge"]) + len(r["reloc"]) for r in a[0])
        plain = [op if not isinstance(op, dict) else ("detect",) for op in ops]
        readds += sum(1 for i, op in enumerate(plain) if op[0] == "add" and ("erase", op[1]) in plain[:i])
    assert detects >= 200 and outputs >= 100 and readds >= 30, (detects, outputs, readds)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_written_case(name):
    world, ops, want, want_state = CASES[name]
    for play in (sk.play_model, sk.play_scan):
        records, states = play(world, ops)
        got = records[-1]
        for key, val in want.items():
            if key == "touched":
                val = sorted(val)
            assert got[key] == val, (name, play.__name__, key, got[key], val)
        for slot, field, value in want_state:
            have = states[-1][slot][field]
            if field in (2, 5):
                have = int(np.frombuffer(have, np.uint32)[0])
            assert have == value, (name, play.__name__, slot, field, have, value)


def test_truncation_table():
    """int(maxCommonWords * 0.8f): the float product, truncated"""
    assert [int(np.float32(m) * np.float32(0.8)) for m in (4, 5, 6, 10, 15)] == [3, 4, 4, 8, 12]


def test_score_against_fsum():
    """The model's score is a sequential double sum of at most 4096 terms |v - w| - |v| - |w|, each of magnitude <= 2 (in fact <= 2 min(v, w)
    for L1-normalised vectors, so the partial sums stay within [-2, 0]).  Each of the n additions rounds a partial sum of magnitude <= 2:
    error <= n * 2^-53 * 2; each term carries two subtraction roundings of its own, <= 2 * 2^-53 * 2 -- in all <= 3 n * 2^-52, and the
    halving is exact.  math.fsum of the exactly computed terms (fractions) is the correctly rounded reference."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for n in (1, 7, 300, 4096):
        w, v1 = sk.bow_vector(rng, 1 << 20, n)
        v2 = rng.random(n) + 0.05; v2 /= v2.sum()
        a = dict(zip(w.tolist(), v1.tolist())); b = dict(zip(w.tolist(), v2.tolist()))
        got = float(km.l1_score(a, b))
        exact = -sum(abs(Fraction(x) - Fraction(y)) - Fraction(x) - Fraction(y) for x, y in zip(v1.tolist(), v2.tolist())) / 2
        assert abs(Fraction(got) - exact) <= 3 * n * Fraction(1, 2 ** 52) / 2, n
        assert abs(got - (-math.fsum(km.l1_terms(a, b)) / 2.0)) <= n * 2.0 ** -52, n
        assert 0.0 <= got <= 1.0


def _wrong_play(world, ops, rule):
    """A compact restatement with one rule switchable to a wrong one: 'unstable' (ties in acc_score ranked latest first), 'ge' (words >=
    minCommonWords), 'connected_listed', 'stale_zero' (a neighbour this query did not score contributes 0).  rule None is the right one."""
    ns = world["n_slots"]
    st = [[0, 0, np.float32(0)] for _ in range(2 * ns)]                       # [slot * 2 + mode] = [query, words, score]
    order = []                                                                # alive slots in add order
    out = []
    for op in ops:
        if not isinstance(op, dict):
            if op[0] == "add":
                order.append(op[1])
            elif op[0] == "erase":
                order.remove(op[1])
            else:
                raise AssertionError("the wrong-rule player knows add and erase only")
            continue
        m, qid = op["mode"], op["id"]
        conn = set() if m == 1 or rule == "connected_listed" else set(op["connected"])
        listed = []
        for w in op["words"].tolist():
            for s in order:
                if w in world["words"][s]:
                    e = st[2 * s + m]
                    if e[0] != qid:
                        e[1] = 0
                        if s not in conn:
                            e[0] = qid; listed.append(s)
                    e[1] += 1
        rec = dict(sharing=[s for s in listed], scored=[], loop=[], merge=[], reloc=[])
        if listed:
            mx = max(st[2 * s + m][1] for s in listed)
            mn = int(np.float32(mx) * np.float32(0.8))
            fresh = []
            for s in listed:
                if st[2 * s + m][1] > mn or (rule == "ge" and st[2 * s + m][1] == mn):
                    qv = dict(zip(op["words"].tolist(), op["values"].tolist())); kv = dict(zip(world["words"][s].tolist(), world["values"][s].tolist()))
                    st[2 * s + m][2] = np.float32(-sum(abs(qv[w] - kv[w]) - qv[w] - kv[w] for w in sorted(qv) if w in kv) / 2.0)   # exact on the dyadic cases
                    fresh.append(s)
            acc_list, best_acc = [], np.float32(0)
            for s in fresh:
                si = st[2 * s + m][2]; acc, best, bs = si, si, s
                for nb in world["neigh"][s][:10]:
                    if nb >= ns or st[2 * nb + m][0] != qid:
                        continue
                    v = st[2 * nb + m][2] if (rule != "stale_zero" or nb in fresh) else np.float32(0)
                    acc = np.float32(acc + v)
                    if v > best:
                        bs, best = nb, v
                acc_list.append((acc, bs)); rec["scored"].append(s)
                best_acc = max(best_acc, acc)
            if m == 1:
                for acc, bs in acc_list:
                    if acc > np.float32(0.75) * best_acc and world["map"][bs] == op["map"] and bs not in rec["reloc"]:
                        rec["reloc"].append(bs)
            else:
                idx = sorted(range(len(acc_list)), key=lambda j: (-float(acc_list[j][0]), -j if rule == "unstable" else j))
                seen = []
                for j in idx:
                    bs = acc_list[j][1]
                    if bs in seen:
                        continue
                    seen.append(bs)
                    if world["map"][bs] == op["map"]:
                        if len(rec["loop"]) < op["n_candidates"]:
                            rec["loop"].append(bs)
                    elif world["map"][bs] not in world["bad_maps"] and len(rec["merge"]) < op["n_candidates"]:
                        rec["merge"].append(bs)
        out.append(rec)
    return out


def _brief(record):
    return dict(sharing=[e[0] for e in record["sharing"]], scored=[e[0] for e in record["scored"]], loop=record["loop"], merge=record["merge"],
                reloc=record["reloc"])


def test_wrong_rules_are_told_apart():
    """every wrong rule changes some list of some hand-written case; the right rule, restated the same compact way, changes none"""
    usable = {n: c for n, c in CASES.items() if all(isinstance(op, dict) or op[0] in ("add", "erase") for op in c[1])}
    assert len(usable) >= 10
    right = {n: [_brief(r) for r in sk.play_model(c[0], c[1])[0]] for n, c in usable.items()}
    for n, c in usable.items():
        assert _wrong_play(c[0], c[1], None) == right[n], n
    told = {}
    for rule in ("unstable", "ge", "connected_listed", "stale_zero"):
        told[rule] = [n for n, c in usable.items() if _wrong_play(c[0], c[1], rule) != right[n]]
        assert told[rule], rule
    assert "ties" in told["unstable"] and "connected" in told["connected_listed"] and "stale_score" in told["stale_zero"]
    assert any(n.startswith("truncation") for n in told["ge"])


def test_update_scripts_cover_every_operation():
    """the scripts tests/test_gpu_kfdb.py::test_update_paths plays hold every update path"""
    ops = sum((sk.make_script(sk.make_world(s, bad_maps=[2] if s % 2 else []), 60, seed=s) for s in (2, 19, 33)), [])
    assert {"add", "erase", "clear_map", "clear", "reset"} <= set(op[0] for op in ops if not isinstance(op, dict))


NEW_SYMBOLS = ("orbhip_kfdb_create", "orbhip_kfdb_destroy", "orbhip_kfdb_add_device", "orbhip_kfdb_add_host", "orbhip_kfdb_erase",
               "orbhip_kfdb_clear_map", "orbhip_kfdb_clear", "orbhip_kfdb_reset_slot", "orbhip_kfdb_get_state_host", "orbhip_kfdb_score_device",
               "orbhip_kfdb_detect_device", "orbhip_kfdb_score_host")


def test_new_symbols_are_declared_exported_and_bound():
    import orbhip
    txt = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name) and getattr(orbhip.lib, name).argtypes is not None, name
    for name in ("kfdb_create", "kfdb_add_device", "kfdb_add_host", "kfdb_erase", "kfdb_clear", "kfdb_clear_map", "kfdb_reset_slot",
                 "kfdb_score_device", "kfdb_detect_device", "kfdb_score_host", "kfdb_get_state"):
        assert callable(getattr(orbhip, name)), name
    assert orbhip.KFDB_NEIGHBOURS == int(re.search(r"#define ORBHIP_KFDB_NEIGHBOURS (\d+)", txt).group(1)) == 10


def test_record_sizes_match_the_header(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "orbhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(orbhip_kfdb_query), '
                   'sizeof(orbhip_kfdb_entry), sizeof(orbhip_kfdb_candidate), sizeof(orbhip_kfdb_slot_state)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    import orbhip
    assert subprocess.check_output([str(exe)], text=True).split() == [str(d.itemsize) for d in (
        orbhip.KFDB_QUERY_DTYPE, orbhip.KFDB_ENTRY_DTYPE, orbhip.KFDB_CANDIDATE_DTYPE, orbhip.KFDB_STATE_DTYPE)]


def test_argument_checks_need_no_device():
    """a NULL database and a bad capacity are refused before anything touches a device, the field named"""
    import orbhip
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.kfdb_create(None, 4, 16)
    assert ei.value.code == orbhip.E_BADARG
    q = np.zeros(1, orbhip.KFDB_QUERY_DTYPE)
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.kfdb_score_device(None, q, 1, 1, 1, 1, None, None, 0, 8, 1, 1)
    assert ei.value.code == orbhip.E_BADARG and "db is NULL" in str(ei.value)
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.kfdb_score_host(None, 1, 0, 0, [1], [1.0])
    assert ei.value.code == orbhip.E_BADARG and "db is NULL" in str(ei.value)
    assert orbhip.lib.orbhip_kfdb_erase(None, 0) == orbhip.E_BADARG and orbhip.lib.orbhip_kfdb_clear(None) == orbhip.E_BADARG


def test_reference_call_lines_compile_against_the_host_class(tmp_path):
    """host/compile_callers_kfdb.cc (the reference's lines LoopClosing.cc:278, :285, :292, :434, :463, :488, Tracking.cc:2634, :2819, :2883,
    KeyFrame.cc:744) builds -Wall -Werror against the host headers, and every KeyFrameDatabase member it calls is defined by
    host/KeyFrameDatabase.cc"""
    host = os.path.join(PKG, "host")
    obj = str(tmp_path / "callers.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(host, "compile_callers_kfdb.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::KeyFrameDatabase::" in ln]
    for member in ("add", "erase", "clear", "clearMap", "DetectNBestCandidates", "DetectRelocalizationCandidates", "SetORBVocabulary"):
        assert any("KeyFrameDatabase::%s(" % member in w for w in wanted), (member, wanted)
    o = str(tmp_path / "kfdb.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-c", "-o", o, os.path.join(host, "KeyFrameDatabase.cc")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined]


@pytest.mark.parametrize("mode", ["tail", "threads"])
def test_host_tail_without_a_device(tmp_path, mode):
    """mode threads: every second call, the first included, comes from a thread of its own that ends right after it -- the object's
    bookkeeping and mutex with several callers, as far as that goes without a device (tests/test_gpu_kfdb.py does it on one).
    The class's host tail (accumulation, rank, selection: rules 5-6) through lib/host_kfdb_smoke's `tail` mode, which feeds it the sharing
    list the device call would have returned -- taken here from the model -- and so needs no GPU.  Outputs and all six fields of every
    keyframe against the model after every call."""
    exe = os.path.join(PKG, "lib", "host_kfdb_smoke")
    assert os.path.exists(exe), "lib/host_kfdb_smoke not built"
    for seed in (3, 12, 31):
        world = sk.make_world(seed, bad_maps=[2] if seed % 3 == 0 else [])
        ops = sk.make_script(world, 50, seed=seed, with_reset=False)
        records, states = sk.play_model(world, ops, clear_zeroes=False)
        script = str(tmp_path / ("s%d.txt" % seed))
        sk.write_script(script, world, ops)
        feed = str(tmp_path / ("f%d.txt" % seed))
        with open(feed, "w") as f:                                            # per detect: counts, then the list and the touched rows
            for r in records:
                f.write("%d %d %d %d\n" % (len(r["sharing"]), r["max_common"], len(r["scored"]), len(r["touched"])))
                for s, w, sc, bits in r["sharing"]:
                    f.write("%d %d %d %d\n" % (s, w, sc, bits))
                for s, w in r["touched"]:
                    f.write("%d %d 0 0\n" % (s, w))
        res = subprocess.run([exe, mode, script, feed], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        got = sk.parse_smoke_output(res.stdout)
        assert len(got) == len(ops)
        it = iter(records)
        for i, op in enumerate(ops):
            want_state = [(s[0], s[1], int(np.frombuffer(s[2], np.uint32)[0]), s[3], s[4], int(np.frombuffer(s[5], np.uint32)[0])) for s in states[i]]
            assert got[i][3] == want_state, (seed, i, op)
            if isinstance(op, dict):
                r = next(it)
                assert (got[i][0], got[i][1], got[i][2]) == (r["loop"], r["merge"], r["reloc"]), (seed, i)
