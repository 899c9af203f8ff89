"""GPU tests of the device-resident KeyFrameDatabase (orbhip_kfdb_*, csrc/kfdb_kernels.hip) and of host/KeyFrameDatabase.cc, bit for bit
against tests/kfdb_model.py (a transcription of the reference's text, not a DBoW2 build): every list, count and float bit pattern, the
stored state of every slot after every call, and output rows beyond the counts untouched."""
import os
import subprocess
import numpy as np
import pytest
import kfdb_cases
import synth_kfdb as sk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_kfdb_smoke")
FILL = 0xA5


class DeviceDB:
    """a world's keyframes in an orbhip_kfdb (keyframe k in slot k), its neighbour table on the device, and batched detect calls"""
    def __init__(self, ctx, world, capacity, max_words, max_list=None, max_conn=16):
        import torch
        import orbhip
        self.torch, self.o, self.ctx, self.world = torch, orbhip, ctx, world
        self.capacity, self.max_words, self.max_conn = capacity, max_words, max_conn
        self.max_list = min(capacity, orbhip.KFDB_MAX_LIST) if max_list is None else max_list
        self.db = orbhip.kfdb_create(ctx, capacity, max_words)
        ns = world["n_slots"]
        neigh = np.full((capacity, orbhip.KFDB_NEIGHBOURS), -1, np.int32)
        for k in range(min(ns, capacity)):
            row = [j if j < ns else -1 for j in world["neigh"][k]][:orbhip.KFDB_NEIGHBOURS]
            neigh[k, :len(row)] = row
        self.d_neigh = torch.from_numpy(neigh).cuda()

    def close(self):
        self.db.close()

    def apply(self, op):
        o, w = self.o, self.world
        if op[0] == "add":
            o.kfdb_add_host(self.db, op[1], w["map"][op[1]], w["words"][op[1]], w["values"][op[1]])
        elif op[0] == "erase":
            o.kfdb_erase(self.db, op[1])
        elif op[0] == "clear_map":
            o.kfdb_clear_map(self.db, op[1])
        elif op[0] == "clear":
            o.kfdb_clear(self.db)
        elif op[0] == "reset":
            o.kfdb_reset_slot(self.db, op[1])

    def detect(self, queries, score_only=False):
        """one call with len(queries) queries -> one record per query, in the models' form; asserts the rows behind the counts untouched"""
        torch, o = self.torch, self.o
        Q, ns = len(queries), self.world["n_slots"]
        stride = max(1, max(len(q["words"]) for q in queries))
        qw = np.zeros((Q, stride), np.int32); qv = np.zeros((Q, stride), np.float64); qn = np.zeros(Q, np.int32)
        conn = np.full((Q, self.max_conn), -1, np.int32); nconn = np.zeros(Q, np.int32)
        rec = np.zeros(Q, o.KFDB_QUERY_DTYPE)
        ncand = max(q["n_candidates"] for q in queries)
        assert all(q["n_candidates"] == ncand for q in queries)
        for i, q in enumerate(queries):
            n = len(q["words"]); qw[i, :n] = q["words"]; qv[i, :n] = q["values"]; qn[i] = n
            c = [j if j < ns else -1 for j in q["connected"]]
            conn[i, :len(c)] = c; nconn[i] = len(c)
            rec[i] = (q["id"], q["map"], q["mode"])
        dev = [torch.from_numpy(a).cuda() for a in (qw, qv, qn, conn, nconn)]
        ML, NC = self.max_list, max(ncand, 1)
        shapes = dict(counts=(Q, 4, 4), list=(Q, ML, 16), scored=(Q, ML, 16), loop=(Q, NC, 4), merge=(Q, NC, 4), ncand=(Q, 2, 4), reloc=(Q, ML, 4), nreloc=(Q, 1, 4))
        out = {k: torch.full(s, FILL, dtype=torch.uint8, device="cuda") for k, s in shapes.items()}
        torch.cuda.synchronize()
        if score_only:
            o.kfdb_score_device(self.db, rec, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), stride, dev[3].data_ptr(), dev[4].data_ptr(),
                                self.max_conn, ML, out["counts"].data_ptr(), out["list"].data_ptr())
        else:
            o.kfdb_detect_device(self.db, rec, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), stride, dev[3].data_ptr(), dev[4].data_ptr(),
                                 self.max_conn, self.d_neigh.data_ptr(), ncand, self.world["bad_maps"], ML, out["counts"].data_ptr(),
                                 out["list"].data_ptr(), out["scored"].data_ptr(), out["loop"].data_ptr(), out["merge"].data_ptr(),
                                 out["ncand"].data_ptr(), out["reloc"].data_ptr(), out["nreloc"].data_ptr())
        self.ctx.synchronize()
        h = {k: v.cpu().numpy() for k, v in out.items()}
        counts = h["counts"].view(np.int32).reshape(Q, 4)
        lst = h["list"].reshape(Q, ML * 16).view(o.KFDB_ENTRY_DTYPE)
        records = []
        for i in range(Q):
            nsh, mx, nsc, nt = (int(x) for x in counts[i])
            assert (h["list"][i, nsh + nt:] == FILL).all(), "list rows behind the counts were written"
            sharing = [(e["slot"], e["words"], e["scored"], e["score"]) for e in lst[i, :nsh]]
            touched = [(e["slot"], e["words"]) for e in lst[i, nsh:nsh + nt]]
            assert all(e["scored"] == 0 and e["score"] == 0 for e in lst[i, nsh:nsh + nt])
            scored, loop, merge, reloc = [], [], [], []
            if score_only:
                assert all((h[k] == FILL).all() for k in ("scored", "loop", "merge", "ncand", "reloc", "nreloc"))
            else:
                sc = h["scored"].reshape(Q, ML * 16).view(o.KFDB_CANDIDATE_DTYPE)[i]
                scored = [(e["slot"], e["score"], e["acc_score"], e["best_slot"]) for e in sc[:nsc]]
                nl, nm = (int(x) for x in h["ncand"].view(np.int32).reshape(Q, 2)[i])
                nr = int(h["nreloc"].view(np.int32).reshape(Q)[i])
                assert nl <= ncand and nm <= ncand and nr <= nsc
                loop = h["loop"].view(np.int32).reshape(Q, NC)[i, :nl].tolist()
                merge = h["merge"].view(np.int32).reshape(Q, NC)[i, :nm].tolist()
                reloc = h["reloc"].view(np.int32).reshape(Q, ML)[i, :nr].tolist()
                assert (h["scored"][i, nsc:] == FILL).all() and (h["loop"][i, nl:] == FILL).all() and (h["merge"][i, nm:] == FILL).all() and (h["reloc"][i, nr:] == FILL).all()
            records.append(sk._record(sharing, touched, mx, scored, loop, merge, reloc))
        return records

    def states(self):
        s = self.o.kfdb_get_state(self.db, 0, min(self.world["n_slots"], self.capacity))
        return [(int(e["query"][0]), int(e["words"][0]), np.float32(e["score"][0]).tobytes(), int(e["query"][1]), int(e["words"][1]),
                 np.float32(e["score"][1]).tobytes()) for e in s]


def _strip(record, score_only):
    return dict(record, scored=[], loop=[], merge=[], reloc=[]) if score_only else record


def _play_device(ctx, world, ops, capacity, max_words, check_states=True, score_only=False, **kw):
    """the script one operation per call against the model: records and, after every operation, every slot's state"""
    want_rec, want_state = sk.play_model(world, ops)
    dev = DeviceDB(ctx, world, capacity, max_words, **kw)
    try:
        it = iter(want_rec)
        n_out = 0
        for i, op in enumerate(ops):
            if isinstance(op, dict):
                got = dev.detect([op], score_only)[0]
                want = _strip(next(it), score_only)
                assert got == want, (i, got, want)
                n_out += len(got["scored"])
            else:
                dev.apply(op)
            if check_states:
                assert dev.states() == want_state[i][:capacity], i
        ctx.check_status()
        return n_out
    finally:
        dev.close()


LENGTHS = [0, 1, 63, 64, 65, 255, 256]


def _length_world(seed, n_slots, vocab):
    world = sk.make_world(seed, n_slots=n_slots, n_extra=2, vocab=vocab, words=(1, 1), dup=0.1, max_neigh=12)
    rng = np.random.default_rng([seed, 5])
    pool = np.sort(rng.choice(vocab, size=600, replace=False))                # a shared pool so that sparse ids still meet
    for k in range(world["n"]):
        world["words"][k], world["values"][k] = sk.bow_vector(rng, vocab, LENGTHS[k % len(LENGTHS)], ids=pool)
    return world, rng, pool


@pytest.mark.parametrize("vocab", [1000, 1 << 20])
@pytest.mark.parametrize("n_slots", [1, 2, 63, 64, 65, 300])
def test_vector_lengths_and_database_sizes(gpu_ctx, n_slots, vocab):
    """capacity 300, max_words 256; database and query vectors of 0, 1, 63, 64, 65, 255 and 256 words over a dense 1000-word vocabulary
    and over ids up to 2^20; 1 to 300 keyframes, so that every launch is ragged"""
    world, rng, pool = _length_world(n_slots * 7 + (vocab > 1000), n_slots, vocab)
    ops = [("add", int(k)) for k in rng.permutation(n_slots)]
    for i, n in enumerate(LENGTHS + [256, 65]):
        q = sk.make_query(world, rng, i % 2, ids=(11 + i,), near=0.0)
        if i < len(LENGTHS):
            q["words"], q["values"] = sk.bow_vector(rng, vocab, n, ids=pool)
        else:                                                                 # a stored vector itself: score 1, every word shared
            j = [k for k in range(n_slots) if len(world["words"][k]) == n]
            if j:
                q["words"], q["values"] = world["words"][j[0]].copy(), world["values"][j[0]].copy()
        ops.append(q)
    n_out = _play_device(gpu_ctx, world, ops, 300, 256)
    assert n_out > 0 or n_slots < 3


def test_4096_words(gpu_ctx):
    """max_words 4096: a database vector and the query both hold 4096 words (the sequential sum at its longest)"""
    rng = np.random.default_rng(9)
    full = sk.bow_vector(rng, 1 << 20, 4096)
    part = (full[0][::3].copy(), full[1][::3] / full[1][::3].sum())
    other = sk.bow_vector(rng, 1 << 20, 4096)
    world = dict(seed=0, n_slots=3, n=3, vocab=1 << 20, n_maps=2, words=[full[0], part[0], other[0]], values=[full[1], part[1], other[1]], map=[0, 1, 0],
                 neigh=[[1], [0, 2], []], bad_maps=[])
    qv = rng.random(4096) + 0.05
    q = dict(op="detect", mode=0, id=5, map=0, words=full[0].copy(), values=qv / qv.sum(), connected=[], n_candidates=3)
    q2 = dict(q, mode=1, id=6, values=full[1].copy())
    n_out = _play_device(gpu_ctx, world, [("add", 0), ("add", 1), ("add", 2), q, q2], 3, 4096)
    assert n_out >= 2


@pytest.mark.parametrize("batch", [1, 3, 17])
def test_batched_calls_equal_single_calls_and_the_model(gpu_ctx, batch):
    """a call with several queries is the function called once per query in index order on the same state: repeated ids and mixed modes
    inside one call included"""
    world = sk.make_world(41, n_slots=40, n_extra=3, vocab=70, bad_maps=[2])
    rng = np.random.default_rng(batch)
    adds = [("add", int(k)) for k in rng.permutation(40)[:33]]
    queries = [sk.make_query(world, rng, int(rng.random() < 0.4), ids=(0, 3, 3, 5, 8)) for _ in range(batch)]
    if batch > 1:
        queries[1] = dict(queries[1], id=queries[0]["id"], mode=queries[0]["mode"])                  # the same id twice in a row
        queries[2] = dict(queries[2], mode=1 - queries[1]["mode"])                                   # and the other mode behind it
        assert len(set((q["id"], q["mode"]) for q in queries)) < batch
    want_rec, want_state = sk.play_model(world, adds + queries)
    one, many = DeviceDB(gpu_ctx, world, 40, 64), DeviceDB(gpu_ctx, world, 40, 64)
    try:
        for op in adds:
            one.apply(op); many.apply(op)
        got_many = many.detect(queries)
        got_one = [one.detect([q])[0] for q in queries]
        assert got_many == want_rec
        assert got_one == want_rec
        assert many.states() == want_state[-1] and one.states() == want_state[-1]
        assert sum(len(r["scored"]) for r in want_rec) > 0
        gpu_ctx.check_status()
    finally:
        one.close(); many.close()


@pytest.mark.parametrize("seed", [2, 19, 33])
def test_update_paths(gpu_ctx, seed):
    """erase, re-add, clear_map, clear and reset_slot between calls: every record and every slot's state after every operation"""
    world = sk.make_world(seed, bad_maps=[2] if seed % 2 else [])
    ops = sk.make_script(world, 60, seed=seed)
    kinds = set(op[0] if not isinstance(op, dict) else "detect" for op in ops)
    assert {"add", "erase", "detect"} <= kinds
    _play_device(gpu_ctx, world, ops, world["n_slots"], 32)


def test_score_device_is_the_first_half(gpu_ctx):
    world = sk.make_world(8)
    ops = sk.make_script(world, 40, seed=8)
    _play_device(gpu_ctx, world, ops, world["n_slots"], 32, score_only=True)


@pytest.mark.parametrize("name", sorted(kfdb_cases.cases()))
def test_hand_written_case_on_the_device(gpu_ctx, name):
    world, ops, want, want_state = kfdb_cases.cases()[name]
    dev = DeviceDB(gpu_ctx, world, max(world["n_slots"], 1), 16)
    try:
        got = None
        for op in ops:
            if isinstance(op, dict):
                got = dev.detect([op])[0]
            else:
                dev.apply(op)
        for key, val in want.items():
            assert got[key] == (sorted(val) if key == "touched" else val), (name, key, got[key], val)
        states = dev.states()
        for slot, field, value in want_state:
            have = states[slot][field]
            assert (int(np.frombuffer(have, np.uint32)[0]) if field in (2, 5) else have) == value, (name, slot, field)
        assert states == sk.play_model(world, ops)[1][-1]
    finally:
        dev.close()


def test_bow_chain_feeds_the_database_on_the_device(gpu_ctx):
    """descriptors -> orbhip_bow_transform_device -> orbhip_bow_vectors_device -> orbhip_kfdb_add_device -> orbhip_kfdb_detect_device with the
    BoW rows never leaving the device; the result equals the model fed with host copies of those rows"""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(77)
    voc = om.make_vocabulary(rng, 8, 3)
    F, MN, MNODE, L, LUP = 12, 256, 256, 3, 1
    n = np.array([0, 1, 63, 64, 65, 200, 256, 256, 130, 90, 256, 180], np.int32)
    base = voc["node_desc"][rng.integers(1, len(voc["node_desc"]), 400)]
    desc = np.zeros((F, MN, 32), np.uint8)
    for f in range(F):
        desc[f, :n[f]] = base[rng.integers(0, 400, n[f])] ^ (rng.integers(0, 256, (n[f], 32), dtype=np.uint8) & rng.integers(0, 256, (n[f], 32), dtype=np.uint8) & rng.integers(0, 256, (n[f], 32), dtype=np.uint8))
    dv = [torch.from_numpy(np.ascontiguousarray(voc[key])).cuda() for key in ("node_desc", "child_start", "child_ids", "node_word", "node_weight")]
    d_desc = torch.from_numpy(desc).cuda(); d_n = torch.from_numpy(n).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    wid, w, nid = z((F, MN), torch.int32), z((F, MN), torch.float64), z((F, MN), torch.int32)
    ni, st, ft, nn = z((F, MNODE), torch.int32), z((F, MNODE + 1), torch.int32), z((F, MN), torch.int32), z((F,), torch.int32)
    bw, bv, nw = z((F, MN), torch.int32), z((F, MN), torch.float64), z((F,), torch.int32)
    torch.cuda.synchronize()
    orbhip.bow_transform_device(gpu_ctx, d_desc.data_ptr(), d_n.data_ptr(), F, MN, MN, [t.data_ptr() for t in dv], L, LUP, wid.data_ptr(), w.data_ptr(), nid.data_ptr())
    orbhip.bow_vectors_device(gpu_ctx, wid.data_ptr(), w.data_ptr(), nid.data_ptr(), d_n.data_ptr(), F, MN, MNODE, ni.data_ptr(), st.data_ptr(), ft.data_ptr(),
                              nn.data_ptr(), bw.data_ptr(), bv.data_ptr(), nw.data_ptr())
    NKF, NQ = 9, 3                                                             # frames 0..8 are keyframes, 9..11 the queries, straight from the rows
    db = orbhip.kfdb_create(gpu_ctx, NKF, MN)
    try:
        for k in range(NKF):
            orbhip.kfdb_add_device(db, k, k % 2, bw.data_ptr() + 4 * MN * k, bv.data_ptr() + 8 * MN * k, nw.data_ptr() + 4 * k)
        neigh = np.full((NKF, 10), -1, np.int32)
        for k in range(NKF):
            neigh[k, :2] = [(k + 1) % NKF, (k + 3) % NKF]
        d_neigh = torch.from_numpy(neigh).cuda()
        rec = np.zeros(NQ, orbhip.KFDB_QUERY_DTYPE)
        rec["id"], rec["map_id"], rec["mode"] = [21, 22, 23], [0, 1, 0], [0, 1, 0]
        counts, ncand, nrel = z((NQ, 4), torch.int32), z((NQ, 2), torch.int32), z((NQ,), torch.int32)
        lst, sc = z((NQ, NKF, 16), torch.uint8), z((NQ, NKF, 16), torch.uint8)
        loop, merge, reloc = z((NQ, 3), torch.int32), z((NQ, 3), torch.int32), z((NQ, NKF), torch.int32)
        orbhip.kfdb_detect_device(db, rec, bw.data_ptr() + 4 * MN * NKF, bv.data_ptr() + 8 * MN * NKF, nw.data_ptr() + 4 * NKF, MN, None, None, 0,
                                  d_neigh.data_ptr(), 3, [], NKF, counts.data_ptr(), lst.data_ptr(), sc.data_ptr(), loop.data_ptr(), merge.data_ptr(),
                                  ncand.data_ptr(), reloc.data_ptr(), nrel.data_ptr())
        gpu_ctx.check_status()
        h_bw, h_bv, h_nw = bw.cpu().numpy(), bv.cpu().numpy(), nw.cpu().numpy()
        assert h_nw[1:].min() >= 1 and h_nw.max() > 64
        world = dict(seed=0, n_slots=NKF, n=NKF, vocab=voc["n_words"], n_maps=2, words=[h_bw[k, :h_nw[k]] for k in range(NKF)],
                     values=[h_bv[k, :h_nw[k]] for k in range(NKF)], map=[k % 2 for k in range(NKF)], neigh=[[(k + 1) % NKF, (k + 3) % NKF] for k in range(NKF)],
                     bad_maps=[])
        ops = [("add", k) for k in range(NKF)] + [dict(op="detect", mode=int(rec["mode"][i]), id=int(rec["id"][i]), map=int(rec["map_id"][i]),
                                                       words=h_bw[NKF + i, :h_nw[NKF + i]], values=h_bv[NKF + i, :h_nw[NKF + i]], connected=[], n_candidates=3)
                                                  for i in range(NQ)]
        want, _ = sk.play_model(world, ops)
        c = counts.cpu().numpy(); e = lst.cpu().numpy().reshape(NQ, NKF * 16).view(orbhip.KFDB_ENTRY_DTYPE)
        s = sc.cpu().numpy().reshape(NQ, NKF * 16).view(orbhip.KFDB_CANDIDATE_DTYPE)
        nc, nr = ncand.cpu().numpy(), nrel.cpu().numpy()
        total = 0
        for i in range(NQ):
            got = sk._record([(x["slot"], x["words"], x["scored"], x["score"]) for x in e[i, :c[i, 0]]], [], c[i, 1],
                             [(x["slot"], x["score"], x["acc_score"], x["best_slot"]) for x in s[i, :c[i, 2]]], loop.cpu().numpy()[i, :nc[i, 0]],
                             merge.cpu().numpy()[i, :nc[i, 1]], reloc.cpu().numpy()[i, :nr[i]])
            assert c[i, 3] == 0 and got == want[i], (i, got, want[i])
            total += len(got["loop"]) + len(got["merge"]) + len(got["reloc"])
        assert total >= 3
    finally:
        db.close()


def test_limits_and_errors(gpu_ctx):
    """argument checks only: nothing here reaches a kernel with an index it could misuse"""
    import torch
    import orbhip
    E = orbhip.OrbHipError

    def raises(code, text, fn, *a):
        with pytest.raises(E) as ei:
            fn(*a)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
    raises(orbhip.E_BADARG, "capacity < 1", orbhip.kfdb_create, gpu_ctx, 0, 16)
    raises(orbhip.E_BADARG, "max_words", orbhip.kfdb_create, gpu_ctx, 4, 4097)
    db = orbhip.kfdb_create(gpu_ctx, 4, 8)
    try:
        w8, v8 = np.arange(8, dtype=np.int32), np.full(8, 0.125)
        raises(orbhip.E_CAPACITY, "nwords > max_words", orbhip.kfdb_add_host, db, 0, 0, np.arange(9), np.full(9, 1 / 9))
        raises(orbhip.E_CAPACITY, "slot outside the capacity", orbhip.kfdb_add_host, db, 4, 0, w8, v8)
        raises(orbhip.E_CAPACITY, "slot outside the capacity", orbhip.kfdb_erase, db, -1)
        for s in range(3):
            orbhip.kfdb_add_host(db, s, 0, w8, v8)
        raises(orbhip.E_BADARG, "slot is alive", orbhip.kfdb_add_host, db, 1, 0, w8, v8)
        # add_device with a count beyond max_words: the status word, the slot stays empty on the device
        d_w = torch.arange(16, dtype=torch.int32, device="cuda"); d_v = torch.full((16,), 1 / 16, dtype=torch.float64, device="cuda")
        d_n = torch.tensor([9], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        orbhip.kfdb_add_device(db, 3, 0, d_w.data_ptr(), d_v.data_ptr(), d_n.data_ptr())
        raises(orbhip.E_CAPACITY, "", gpu_ctx.check_status)
        assert orbhip.kfdb_get_state(db)[3]["alive"] == 0
        rec = np.zeros(2, orbhip.KFDB_QUERY_DTYPE); rec["id"] = [4, 5]
        qw = torch.arange(16, dtype=torch.int32, device="cuda").reshape(2, 8) % 8
        qv = torch.full((2, 8), 0.125, dtype=torch.float64, device="cuda")
        out = lambda *shape: torch.full(shape, FILL, dtype=torch.uint8, device="cuda")

        def score(qn, max_list, records=rec):
            counts, lst = out(2, 16), out(2, max(min(max_list, 8), 1) * 16)
            d_qn = torch.tensor(qn, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            orbhip.kfdb_score_device(db, records, qw.data_ptr(), qv.data_ptr(), d_qn.data_ptr(), 8, None, None, 0, max_list, counts.data_ptr(), lst.data_ptr())
            gpu_ctx.synchronize()
            return counts.cpu().numpy().view(np.int32).reshape(2, 4), lst.cpu().numpy()
        # a query vector longer than max_words: status word, zero counts, nothing else written, state untouched; its neighbour is served
        before = orbhip.kfdb_get_state(db).copy()
        counts, lst = score([9, 8], 4)
        raises(orbhip.E_CAPACITY, "", gpu_ctx.check_status)
        assert counts[0].tolist() == [0, 0, 0, 0] and (lst[0] == FILL).all() and counts[1].tolist() == [3, 8, 3, 0]
        after = orbhip.kfdb_get_state(db)
        assert (after["query"][:, 0] == 5).sum() == 3 and (before["query"] == 0).all()
        # a list longer than max_list: status word and zero counts for that query
        rec["id"] = [6, 7]
        counts, lst = score([8, 0], 2)
        raises(orbhip.E_CAPACITY, "", gpu_ctx.check_status)
        assert counts.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]] and (lst == FILL).all()
        raises(orbhip.E_CAPACITY, "max_list", score, [8, 8], 4097)
        raises(orbhip.E_CAPACITY, "max_list", score, [8, 8], 0)
        bad = rec.copy(); bad["mode"][1] = 2
        raises(orbhip.E_BADARG, "mode", score, [8, 8], 4, bad)
        d_qn = torch.tensor([8, 8], dtype=torch.int32, device="cuda"); d_neigh = torch.full((4, 10), -1, dtype=torch.int32, device="cuda")
        o = [out(2, 64) for _ in range(8)]
        torch.cuda.synchronize()
        raises(orbhip.E_BADARG, "n_candidates < 0", orbhip.kfdb_detect_device, db, rec, qw.data_ptr(), qv.data_ptr(), d_qn.data_ptr(), 8, None, None, 0,
               d_neigh.data_ptr(), -1, [], 4, *[t.data_ptr() for t in o])
        raises(orbhip.E_BADARG, "d_neighbours is NULL", orbhip.kfdb_detect_device, db, rec, qw.data_ptr(), qv.data_ptr(), d_qn.data_ptr(), 8, None, None, 0,
               None, 3, [], 4, *[t.data_ptr() for t in o])
        raises(orbhip.E_BADARG, "db is NULL", orbhip.kfdb_detect_device, None, rec, qw.data_ptr(), qv.data_ptr(), d_qn.data_ptr(), 8, None, None, 0,
               d_neigh.data_ptr(), 3, [], 4, *[t.data_ptr() for t in o])
        raises(orbhip.E_CAPACITY, "nwords > max_words", orbhip.kfdb_score_host, db, 9, 0, 0, np.arange(9), np.full(9, 1 / 9))
        c, lst, touched = orbhip.kfdb_score_host(db, 9, 0, 1, w8, v8)
        assert c.tolist() == [3, 8, 3, 0] and lst["slot"].tolist() == [0, 1, 2] and (lst["score"] == 1).all() and len(touched) == 0
        gpu_ctx.check_status()
    finally:
        db.close()


def _class_script():
    world = sk.make_world(57, n_slots=30, n_extra=3, vocab=64, n_maps=3, bad_maps=[2])
    ops = sk.make_script(world, 90, seed=4, with_reset=False)
    assert sum(isinstance(op, dict) for op in ops) >= 40 and len(set(world["map"])) == 3
    return world, ops


@pytest.mark.parametrize("mode", ["run", "threads"])
def test_class_through_the_smoke_driver(gpu_ctx, tmp_path, mode):
    """mode threads: every second call, the first included, comes from a thread that ends right after it, while another thread keeps ITS
    thread context busy with a database of its own and checks every answer: the object must own its context -- on the first caller's it
    would outlive it, and share arenas with that thread's other work.
    host/KeyFrameDatabase.cc: a script of 90 operations with more than 40 Detect... calls on 3 maps (NBest with nNumCandidates = 3);
    result vectors and all six fields of every keyframe against the model after every call"""
    world, ops = _class_script()
    records, states = sk.play_model(world, ops, clear_zeroes=False)
    script = str(tmp_path / "script.txt")
    sk.write_script(script, world, ops)
    res = subprocess.run([EXE, mode, script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert mode == "run" or "all answers right" in res.stderr
    got = sk.parse_smoke_output(res.stdout)
    assert len(got) == len(ops)
    it = iter(records)
    found = 0
    for i, op in enumerate(ops):
        want_state = [(s[0], s[1], int(np.frombuffer(s[2], np.uint32)[0]), s[3], s[4], int(np.frombuffer(s[5], np.uint32)[0])) for s in states[i]]
        assert got[i][3] == want_state, (i, op)
        if isinstance(op, dict):
            r = next(it)
            assert (got[i][0], got[i][1], got[i][2]) == (r["loop"], r["merge"], r["reloc"]), i
            found += len(r["loop"]) + len(r["merge"]) + len(r["reloc"])
    assert found >= 20


def test_class_without_a_usable_device(tmp_path):
    """ORBHIP_DEVICE naming no device: one message on stderr, empty results, the keyframes' fields untouched -- no CPU fallback"""
    world, ops = _class_script()
    script = str(tmp_path / "script.txt")
    sk.write_script(script, world, ops[:40])
    res = subprocess.run([EXE, "run", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=dict(os.environ, ORBHIP_DEVICE="4096"))
    assert res.returncode == 0
    assert res.stderr.count("no device context") == 1 and "no CPU fallback" in res.stderr
    for loop, merge, reloc, states in sk.parse_smoke_output(res.stdout):
        assert loop == [] and merge == [] and reloc == [] and all(s == (0, 0, 0, 0, 0, 0) for s in states)
