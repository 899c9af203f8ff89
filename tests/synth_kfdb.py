"""Seeded worlds and call scripts for the KeyFrameDatabase tests: a vocabulary, L1-normalised sparse BoW vectors, maps, covisibility lists,
and a script of add / erase / clear_map / clear / reset / Detect... calls; and the two players that run a script through kfdb_model.py
(objects + inverted file) and kfdb_scan_model.py (arrays + order key) and return what each call did in one common, comparable form.
Keyframe k of a world lives in slot k; keyframes at index >= n_slots never enter the database (neighbours / connected keyframes without
a slot)."""
import re
import numpy as np
import kfdb_model as km
import kfdb_scan_model as ks


def bow_vector(rng, vocab, n, ids=None):
    """n distinct ascending word ids below `vocab` (or drawn from `ids`) with positive values summing to 1"""
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float64)
    w = np.sort(rng.choice(vocab, size=n, replace=False) if ids is None else rng.choice(ids, size=n, replace=False)).astype(np.int32)
    v = rng.random(n) + 0.05
    return w, v / v.sum()


def make_world(seed, n_slots=24, n_extra=3, vocab=60, n_maps=3, words=(2, 14), bad_maps=(), dup=0.15, max_neigh=12):
    rng = np.random.default_rng(seed)
    n = n_slots + n_extra
    W, V, M = [], [], []
    for k in range(n):
        if k and rng.random() < dup:                                           # a duplicate vector: equal scores, ties in acc_score
            j = int(rng.integers(k)); W.append(W[j].copy()); V.append(V[j].copy())
        else:
            w, v = bow_vector(rng, vocab, int(rng.integers(words[0], min(words[1], vocab) + 1)))
            W.append(w); V.append(v)
        M.append(int(rng.integers(n_maps)))
    neigh = [[int(x) for x in rng.choice(n, size=int(rng.integers(0, min(max_neigh, n - 1) + 1)), replace=False) if x != k] for k in range(n)]
    return dict(seed=seed, n_slots=n_slots, n=n, vocab=vocab, n_maps=n_maps, words=W, values=V, map=M, neigh=neigh, bad_maps=list(bad_maps), rng=rng)


def make_query(world, rng, mode, ids=(0, 1, 2, 3, 7, 7, 9), near=0.7, n_candidates=3, max_words=None):
    n = world["n"]
    if rng.random() < near:                                                    # a perturbed copy of a keyframe's vector: many shared words
        j = int(rng.integers(n))
        keep = rng.random(len(world["words"][j])) < 0.8
        w = world["words"][j][keep]
        extra = np.setdiff1d(rng.choice(world["vocab"], size=min(4, world["vocab"]), replace=False), world["words"][j]).astype(np.int32)
        w = np.sort(np.concatenate([w, extra])).astype(np.int32)
        if max_words is not None:
            w = w[:max_words]
        v = rng.random(len(w)) + 0.05
        v = v / v.sum() if len(w) else v
    else:
        hi = min(14, world["vocab"]) if max_words is None else min(14, world["vocab"], max_words)
        w, v = bow_vector(rng, world["vocab"], int(rng.integers(0, hi + 1)))
    conn = [int(x) for x in rng.choice(n, size=int(rng.integers(0, min(6, n) + 1)), replace=False)] if mode == 0 else []
    return dict(op="detect", mode=mode, id=int(rng.choice(ids)), map=int(rng.integers(world["n_maps"])), words=w, values=v, connected=conn,
                n_candidates=n_candidates)


def make_script(world, n_calls, seed=0, p_detect=0.45, first_adds=None, with_reset=True):
    """ops: ("add", k) ("erase", k) ("clear_map", m) ("clear",) ("reset", k) and detect dicts; erased keyframes are added again later"""
    rng = np.random.default_rng([world["seed"], seed, 77])
    ns = world["n_slots"]
    indb = set()
    ops = []
    for k in rng.permutation(ns)[:ns * 2 // 3 if first_adds is None else first_adds]:
        ops.append(("add", int(k))); indb.add(int(k))
    while len(ops) < n_calls:
        u = rng.random()
        if u < p_detect:
            ops.append(make_query(world, rng, int(rng.random() < 0.4)))
        elif u < p_detect + 0.2 and len(indb) < ns:
            k = int(rng.choice(sorted(set(range(ns)) - indb))); ops.append(("add", k)); indb.add(k)
        elif u < p_detect + 0.4 and indb:
            k = int(rng.choice(sorted(indb))); ops.append(("erase", k)); indb.discard(k)
        elif u < p_detect + 0.45:
            m = int(rng.integers(world["n_maps"])); ops.append(("clear_map", m)); indb = {k for k in indb if world["map"][k] != m}
        elif u < p_detect + 0.47:
            ops.append(("clear",)); indb = set()
        elif len(indb) < ns and with_reset:
            ops.append(("reset", int(rng.choice(sorted(set(range(ns)) - indb)))))
    return ops


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def _record(sharing, touched, max_common, scored, loop, merge, reloc):
    """one comparable record: slots, ints, float bit patterns"""
    return dict(sharing=[(int(s), int(w), int(sc), f32bits(v)) for s, w, sc, v in sharing], touched=sorted((int(s), int(w)) for s, w in touched),
                max_common=int(max_common), scored=[(int(s), f32bits(si), f32bits(acc), int(b)) for s, si, acc, b in scored],
                loop=[int(x) for x in loop], merge=[int(x) for x in merge], reloc=[int(x) for x in reloc])


def play_model(world, ops, clear_zeroes=True):
    """-> per detect op a record, and the state of every slotted keyframe after each op.  clear_zeroes: "clear" is orbhip_kfdb_clear, which
    zeroes the state with the slots; False: the reference's clear(), which leaves the keyframes' fields alone (the host class)"""
    maps = [km.Map(m, m in world["bad_maps"]) for m in range(world["n_maps"])]
    kfs = [km.KeyFrame(1000 + k, zip(world["words"][k], world["values"][k]), maps[world["map"][k]], k if k < world["n_slots"] else None)
           for k in range(world["n"])]
    for k, kf in enumerate(kfs):
        kf.neighbours = [kfs[j] for j in world["neigh"][k]]
    db = km.KeyFrameDatabase()
    records, states, indb = [], [], set()
    for op in ops:
        if isinstance(op, dict):
            q = km.KeyFrame(op["id"], zip(op["words"], op["values"]), maps[op["map"]])
            q.connected = set(kfs[j] for j in op["connected"])
            r = db.DetectNBestCandidates(q, op["n_candidates"]) if op["mode"] == 0 else db.DetectRelocalizationCandidates(q, maps[op["map"]])
            listed = set(id(k) for k in r.sharing)
            scored = {id(k): si for k, si, _, _ in r.scored}
            fld = "mnPlaceRecognitionWords" if op["mode"] == 0 else "mnRelocWords"
            sharing = [(k.slot, getattr(k, fld), 1 if id(k) in scored else 0, scored.get(id(k), 0.0)) for k in r.sharing]
            # met in the inverted file without being listed: connected keyframes and repeated ids
            touched = [(k, getattr(kfs[k], fld)) for k in sorted(indb) if id(kfs[k]) not in listed and set(kfs[k].mBowVec) & set(q.mBowVec)]
            records.append(_record(sharing, touched, r.max_common, [(k.slot, si, acc, b.slot if b.slot is not None else -1) for k, si, acc, b in r.scored],
                                   [k.slot for k in r.loop], [k.slot for k in r.merge], [k.slot for k in r.reloc]))
        elif op[0] == "add":
            db.add(kfs[op[1]]); indb.add(op[1])
        elif op[0] == "erase":
            db.erase(kfs[op[1]]); indb.discard(op[1])
        elif op[0] == "clear_map":
            db.clearMap(maps[op[1]]); indb = {k for k in indb if world["map"][k] != op[1]}
        elif op[0] == "clear":
            db.clear(); indb = set()
            for kf in kfs if clear_zeroes else []:
                kf.reset_state()                                               # orbhip_kfdb_clear zeroes the state with the slots
        elif op[0] == "reset":
            kfs[op[1]].reset_state()
        states.append([kf.state() for kf in kfs[:world["n_slots"]]])
    return records, states


def play_scan(world, ops):
    ns = world["n_slots"]
    db = ks.ScanDatabase(ns)
    neigh = {k: [j if j < ns else -1 for j in world["neigh"][k]] for k in range(ns)}
    records, states = [], []
    for op in ops:
        if isinstance(op, dict):
            o = db.detect(op["id"], op["map"], op["mode"], op["words"], op["values"], [j if j < ns else -1 for j in op["connected"]], neigh,
                          op["n_candidates"], world["bad_maps"])
            records.append(_record(o["sharing"], o["touched"], o["max_common"], o["scored"], o["loop"], o["merge"], o["reloc"]))
        elif op[0] == "add":
            db.add(op[1], world["map"][op[1]], world["words"][op[1]], world["values"][op[1]])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear_map":
            db.clear_map(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "reset":
            db.reset_slot(op[1])
        states.append([(int(db.query[s, 0]), int(db.nwords[s, 0]), np.float32(db.score[s, 0]).tobytes(), int(db.query[s, 1]), int(db.nwords[s, 1]),
                        np.float32(db.score[s, 1]).tobytes()) for s in range(ns)])
    return records, states


def write_script(path, world, ops):
    """the flat-file script lib/host_kfdb_smoke reads (host/host_kfdb_smoke.cc)"""
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (world["n"], world["n_slots"], world["n_maps"]))
        f.write(" ".join(str(int(m in world["bad_maps"])) for m in range(world["n_maps"])) + "\n")
        for k in range(world["n"]):
            f.write("%d %d" % (world["map"][k], len(world["words"][k])))
            for w, v in zip(world["words"][k].tolist(), world["values"][k].tolist()):
                f.write(" %d %s" % (w, float(v).hex()))
            f.write(" %d %s\n" % (len(world["neigh"][k]), " ".join(str(j) for j in world["neigh"][k])))
        f.write("%d\n" % len(ops))
        for op in ops:
            if isinstance(op, dict):
                f.write("%s %d %d %d %d" % ("nbest" if op["mode"] == 0 else "reloc", op["id"], op["map"], op["n_candidates"], len(op["words"])))
                for w, v in zip(op["words"].tolist(), op["values"].tolist()):
                    f.write(" %d %s" % (w, float(v).hex()))
                f.write(" %d %s\n" % (len(op["connected"]), " ".join(str(j) for j in op["connected"])))
            else:
                f.write(" ".join(str(x) for x in op) + "\n")


def parse_smoke_output(text):
    """-> per operation (loop, merge, reloc, states [n_slots][6]) as lib/host_kfdb_smoke prints them"""
    out = []
    for block in re.split(r"(?m)^op ", text.strip())[1:]:
        lines = block.strip().splitlines()
        lists = {}
        for ln in lines[1:4]:
            p = ln.split()
            lists[p[0]] = [int(x) for x in p[1:]]
        states = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[4:]]
        out.append((lists["loop"], lists["merge"], lists["reloc"], states))
    return out
