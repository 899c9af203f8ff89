#!/usr/bin/env python3
"""Call times of the device KeyFrameDatabase (GPU box): orbhip_kfdb_detect_device with 1 and with 64 queries against a database of 4096
keyframes x 1000 words (vocabulary 20000, so a random keyframe shares about 50 words with a query; every query is a stored keyframe's
vector seen again, half of them place recognition, half relocalisation).  Host clock around call + synchronise, warm-up first, every
repetition under a fresh query id (a repeated id lists nothing).  --cluster C: the keyframes come in runs of C views of one place (each
keeps about 95 % of the place's words), so that a query scores about C keyframes whose covisibility neighbours are scored too, instead
of one.  --reps N; --only Q: one batch size alone; --json PATH writes the result there as well."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import numpy as np
import torch
import orbhip

ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=4096); ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--vocabulary", type=int, default=20000); ap.add_argument("--reps", type=int, default=30); ap.add_argument("--json", default=None); ap.add_argument("--cluster", type=int, default=1)
ap.add_argument("--only", type=int, default=0, help="time this batch size alone (for a kernel trace)")
a = ap.parse_args()
K, W, V = a.keyframes, a.words, a.vocabulary
rng = np.random.default_rng(3)
ctx = orbhip.Context(0)
db = orbhip.kfdb_create(ctx, K, W)
words = np.zeros((K, W), np.int32); values = np.zeros((K, W))
t0 = time.perf_counter()
for k in range(K):
    if k % a.cluster == 0:
        place = rng.choice(V, size=W, replace=False)
    w = place.copy()
    if a.cluster > 1:                                       # another view of the place: about 5 % of its words replaced
        swap = rng.random(W) < 0.05
        w[swap] = rng.choice(np.setdiff1d(np.arange(V), place), size=int(swap.sum()), replace=False)
    words[k] = np.sort(w); v = rng.random(W) + 0.05; values[k] = v / v.sum()
    orbhip.kfdb_add_host(db, k, k % 4 == 3, words[k], values[k])
ctx.synchronize()
neigh = np.full((K, 10), -1, np.int32)
for k in range(K):
    nb = [k - j for j in range(1, 11) if k - j >= 0]; neigh[k, :len(nb)] = nb
d_neigh = torch.from_numpy(neigh).cuda()
out = dict(keyframes=K, words=W, vocabulary=V, reps=a.reps, cluster=a.cluster)
next_id = [1]


def run(Q, reps):
    pick = rng.integers(0, K, Q)
    d_qw = torch.from_numpy(words[pick]).cuda(); d_qv = torch.from_numpy(values[pick]).cuda(); d_qn = torch.full((Q,), W, dtype=torch.int32, device="cuda")
    ML = 4096
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    counts, lst, sc, loop, merge, nc, rl, nr = z(Q, 4), z(Q, ML, 4), z(Q, ML, 4), z(Q, 3), z(Q, 3), z(Q, 2), z(Q, ML), z(Q)
    times = []
    for it in range(reps + 5):
        rec = np.zeros(Q, orbhip.KFDB_QUERY_DTYPE)
        rec["id"] = np.arange(next_id[0], next_id[0] + Q); next_id[0] += Q
        rec["mode"] = np.arange(Q) % 2
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        orbhip.kfdb_detect_device(db, rec, d_qw.data_ptr(), d_qv.data_ptr(), d_qn.data_ptr(), W, None, None, 0, d_neigh.data_ptr(), 3, [], ML,
                                  counts.data_ptr(), lst.data_ptr(), sc.data_ptr(), loop.data_ptr(), merge.data_ptr(), nc.data_ptr(), rl.data_ptr(), nr.data_ptr())
        ctx.synchronize()
        if it >= 5:
            times.append((time.perf_counter() - t0) * 1e3)
    ctx.check_status()
    c = counts.cpu().numpy()
    t = np.sort(times)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t[0]), 4), max_ms=round(float(t[-1]), 4), mean_sharing=float(c[:, 0].mean()),
                mean_scored=float(c[:, 2].mean()), candidates=int(nc.sum().item() + nr.sum().item()))


for Q in ([a.only] if a.only else [1, 64]):
    out["detect_%d_quer%s" % (Q, "y" if Q == 1 else "ies")] = run(Q, a.reps)
db.close()
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
