"""Closed form of DistributeOctTree (ORBextractor.cc:537-761): the model the table form of k_octree is written against.

Every full pass of the reference splits exactly the nodes the pass before created, and a node's box depends only on its root and its
quadrant digits.  So the path of a key (root, d1, d2, ...) follows from the key alone, and everything the subdivision loop decides
follows from per-depth COUNT TABLES indexed by path prefix:

  * the list size after pass t is the number of non-empty depth-t prefixes (a single-key node persists and stays one prefix), nToExpand
    is the number of depth-t prefixes with more than one key: the stop tests of ORBextractor.cc:661/665 need nothing else;
  * after pass T the list is (generation T), then the single-key nodes of generation T-1 in their order, ... down to the roots;
    generation t = the non-empty depth-t prefixes whose parent prefix holds more than one key;
  * inside generation t the order is a digit-wise comparison, root first: the digit at distance i from the LAST one is descending when i
    is even (push_front of n1..n4) and ascending when i is odd (the parents were reversed once more); the root is descending when t is
    odd.  With the descending digits complemented (XOR 0x3333... on the digit string, nIni-1-root), ascending code IS list order;
  * the final phase (ORBextractor.cc:671-735) is node-level work: its child counts are the deeper tables.

octree_table() keeps the tables sparse (dictionaries), so that it has no depth limit of its own; `dmax` makes it give up (return None) exactly
where the kernel with tables down to depth dmax hands the list to the iterative form.
"""
import math
from collections import Counter

import numpy as np

ORDER_MASK = 0x3333333333333333

# Test-only switches: each makes the closed form subtly wrong in one rule, so that tests/test_octree_table_model.py can show that the shared case
# set tells the wrong form from the right one.  Nothing but that test passes `mutate`.
MUTATIONS = ("no_digit_complement",        # generation order without the complement of the digits at even distance from the last one
             "no_root_reversal",           # the root ascending at odd depth too
             "final_ties_descending")      # final phase ordered by count alone, equal counts by descending list position


def order_code(raw, d, n_ini, mutate=None):
    """Position code of the depth-d prefix `raw` (root * 4^d + digits) inside generation d: ascending code = list order."""
    root, dig = raw >> (2 * d), raw & ((1 << (2 * d)) - 1)
    if d & 1 and mutate != "no_root_reversal":
        root = n_ini - 1 - root
    if mutate != "no_digit_complement":
        dig ^= ORDER_MASK & ((1 << (2 * d)) - 1)
    return (root << (2 * d)) | dig


class _Paths:
    """Per-key path prefixes, one depth at a time, and their count tables."""

    def __init__(self, xs, ys, W, H):
        xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
        self.xs, self.ys = xs, ys
        self.n_ini = int(math.floor(float(np.float32(W) / np.float32(H)) + 0.5))            # roundf, ORBextractor.cc:541
        hx = np.float32(W) / np.float32(self.n_ini)
        r = (xs.astype(np.float32) / hx).astype(np.int64)                                   # ORBextractor.cc:568
        i = np.arange(self.n_ini + 1, dtype=np.float32)
        edge = (hx * i).astype(np.int64)                                                    # ORBextractor.cc:555-556
        self.x0, self.x1 = edge[r].copy(), edge[r + 1].copy()
        self.y0, self.y1 = np.zeros_like(xs), np.full_like(xs, H)
        self.path = [r]
        self.tab = [Counter(r.tolist())]

    def _extend(self):
        mx = self.x0 + ((self.x1 - self.x0 + 1) >> 1)                                       # DivideNode: ceil(half), ORBextractor.cc:481-482
        my = self.y0 + ((self.y1 - self.y0 + 1) >> 1)
        right, low = self.xs >= mx, self.ys >= my
        self.x0 = np.where(right, mx, self.x0); self.x1 = np.where(right, self.x1, mx)
        self.y0 = np.where(low, my, self.y0); self.y1 = np.where(low, self.y1, my)
        p = self.path[-1] * 4 + right.astype(np.int64) + 2 * low.astype(np.int64)
        assert len(self.path) < 29
        self.path.append(p)
        self.tab.append(Counter(p.tolist()))

    def table(self, d):
        while len(self.tab) <= d:
            self._extend()
        return self.tab[d]


def octree_table(xs, ys, ss, min_x, max_x, min_y, max_y, n_features, dmax=None, info=None, mutate=None):
    """Kept candidate indices in list order, as oracle_bind.octree gives them; None where tables down to depth `dmax` do not reach.
    `info` (a dict) receives what the tree did: T, quirk, final, final_iters, mid_stop, tie, depth.  `mutate`: one of MUTATIONS (test only)."""
    assert mutate is None or mutate in MUTATIONS
    info = {} if info is None else info
    info.update(T=0, quirk=False, final=False, final_iters=0, mid_stop=False, tie=False, depth=0)
    K, N = len(xs), n_features
    if K == 0:
        return np.zeros(0, np.int32)
    P = _Paths(xs, ys, max_x - min_x, max_y - min_y)
    n_ini = P.n_ini

    def tab(d):
        return None if (dmax is not None and d > dmax) else P.table(d)

    # ---- stop depth from the per-depth counts (ORBextractor.cc:593-665)
    t, prev = 0, len(P.table(0))
    while True:
        t += 1
        c = tab(t)
        if c is None:
            return None
        size = len(c)
        nexp = sum(1 for v in c.values() if v > 1)
        if size >= N or size == prev:
            final = False
            info["quirk"] = size == prev and size < N and nexp > 0
            break
        if size + 3 * nexp > N:
            final = True
            break
        if nexp == 0:                                                    # nothing left to split: the next pass would change nothing
            final = False
            break
        prev = size
    T = t
    info.update(T=T, final=final)
    # ---- the list after pass T: generation T, then the single-key nodes of the generations before it, each in its own order
    nd, nraw, ncnt = [], [], []
    for d in range(T, -1, -1):
        c = P.table(d)
        up = P.table(d - 1) if d else None
        here = [raw for raw, v in c.items() if (d == 0 or up[raw >> 2] > 1) and (d == T or v == 1)]
        here.sort(key=lambda raw: order_code(raw, d, n_ini, mutate))
        for raw in here:
            nd.append(d); nraw.append(raw); ncnt.append(c[raw])
        if d == T:
            front = len(here)
    # ---- final phase on nodes alone (ORBextractor.cc:671-735)
    while final:
        size = len(nd)
        cand = [p for p in range(front) if ncnt[p] > 1]
        if not cand:
            break                                                        # size == prevSize
        cand.sort(key=lambda p: (-ncnt[p], -p if mutate == "final_ties_descending" else p))   # (size desc, creation desc) == (size desc, list position asc)
        c = tab(nd[cand[0]] + 1)                                         # every candidate is one generation: same depth
        if c is None:
            return None
        done, kids = [], []
        info["final_iters"] += 1
        info["tie"] = info["tie"] or len({ncnt[p] for p in cand}) < len(cand)
        for p in cand:
            ch = [(nd[p] + 1, 4 * nraw[p] + q, c[4 * nraw[p] + q]) for q in (3, 2, 1, 0) if c.get(4 * nraw[p] + q, 0) > 0]
            kids = ch + kids                                             # push_front: the later parent's children land in front
            done.append(p)
            size += len(ch) - 1
            if size >= N:
                info["mid_stop"] = len(done) < len(cand)
                break
        gone = set(done)
        keep = [p for p in range(len(nd)) if p not in gone]
        new = kids + [(nd[p], nraw[p], ncnt[p]) for p in keep]
        grown = len(new) != len(nd)
        nd, nraw, ncnt = [list(v) for v in zip(*new)]
        front = len(kids)
        if len(nd) >= N or not grown:
            break
    # ---- every key finds its node through its own path; best response per node, first in list order wins (ORBextractor.cc:739-758)
    pos = {(d, raw): p for p, (d, raw) in enumerate(zip(nd, nraw))}
    dfin = max(nd)
    info["depth"] = dfin
    best = [-1] * len(nd)
    for k in range(K):
        for d in range(dfin + 1):
            p = pos.get((d, int(P.path[d][k])))
            if p is not None:
                break
        assert p is not None
        if best[p] < 0 or ss[k] > ss[best[p]]:
            best[p] = k
    return np.asarray(best, np.int32)


# ------------------------------------------------------------------ cases, shared by the CPU and the GPU tests
GEOMETRIES = [(300, 300), (608, 448), (500, 250), (600, 200), (640, 160)]          # (W, H) of the detection area: nIni 1, 1, 2, 3, 4


def random_case(kind, seed, geometry=None, quota=None):
    """kind 0 uniform, 1 clustered, 2 tight blocks.  Returns dict(W, H, N, xs, ys, ss); candidates are distinct pixels.
    `geometry` = (W, H) and `quota` replace the drawn detection area and quota; the draws themselves are made all the same, so that a seed
    gives the same list shape with and without them."""
    rng = np.random.RandomState(1000 * kind + seed)
    W, H = GEOMETRIES[rng.randint(len(GEOMETRIES))]
    N = int(rng.choice([12, 20, 37, 60, 100, 217, 400, 1000]))
    if geometry is not None:
        W, H = geometry
    if quota is not None:
        N = int(quota)
    K = int(rng.choice([1, 2, 5, 40, 150, 400, 900, 2500]))
    if kind == 0:
        x, y = rng.randint(0, W, K), rng.randint(0, H, K)
    elif kind == 1:
        nc = rng.randint(1, 7)
        cx, cy, sg = rng.randint(0, W, nc), rng.randint(0, H, nc), rng.choice([3, 8, 25, 60], nc)
        w = rng.randint(nc, size=K)
        x = np.clip(np.round(cx[w] + sg[w] * rng.randn(K)), 0, W - 1).astype(int)
        y = np.clip(np.round(cy[w] + sg[w] * rng.randn(K)), 0, H - 1).astype(int)
    else:
        nb = rng.randint(1, 4)
        side = int(rng.choice([6, 12, 20, 40]))
        bx, by = rng.randint(0, W - side, nb), rng.randint(0, H - side, nb)
        w = rng.randint(nb, size=K)
        x, y = bx[w] + rng.randint(0, side, K), by[w] + rng.randint(0, side, K)
    _, first = np.unique(y * 4096 + x, return_index=True)                       # NMS never keeps one pixel twice
    first.sort()
    x, y = x[first], y[first]
    s = rng.randint(7, 256 if seed % 3 else 12, len(x))                          # every third case: few distinct scores (ties inside a node)
    return dict(W=W, H=H, N=N, xs=x.astype(np.int32), ys=y.astype(np.int32), ss=s.astype(np.int32))


def _search(W, H, N, K, want, side=None, seeds=4000, base=0):
    """First seeded point set whose tree has the wanted properties (per the model's own record; the tests check it against the oracle)."""
    for seed in range(seeds):
        rng = np.random.RandomState(base + seed)
        if side:
            bx, by = rng.randint(0, W - side), rng.randint(0, H - side)
            x, y = bx + rng.randint(0, side, K), by + rng.randint(0, side, K)
        else:
            x, y = rng.randint(0, W, K), rng.randint(0, H, K)
        _, first = np.unique(y * 4096 + x, return_index=True)
        first.sort()
        x, y = x[first], y[first]
        s = rng.randint(7, 256, len(x))
        info = {}
        octree_table(x, y, s, 16, 16 + W, 16, 16 + H, N, info=info)
        if want(info):
            return dict(W=W, H=H, N=N, xs=x.astype(np.int32), ys=y.astype(np.int32), ss=s.astype(np.int32))
    raise AssertionError("no seed gives the wanted tree")


def table_depth(n_ini, quotas):
    """Depth of the deepest count table of k_octree_tab (orb_octree_dmax): the tables share the kernel's LDS with 9 words per node slot."""
    nc = max(max(q + 16, 4 * n_ini + 4) for q in quotas)
    d = 0
    while d < 7 and n_ini * ((4 ** (d + 2) - 1) // 3) <= 7 * nc:
        d += 1
    return d if d >= 2 else 0


def hand_cases():
    """name -> case: the smallest inputs at which the table form can go wrong."""
    c = {}
    i32 = lambda *v: np.asarray(v, np.int32)
    c["empty"] = dict(W=300, H=300, N=20, xs=i32(), ys=i32(), ss=i32())
    c["one_key"] = dict(W=300, H=300, N=20, xs=i32(123), ys=i32(45), ss=i32(99))
    # two keys that only the split of the depth-4 box separates (300 -> 150 -> 75 -> 38 -> 19 wide), each pass before it splits one other key off
    # the same with the split at depth 3, the deepest table of a small quota
    c["two_keys_last_table"] = dict(W=300, H=300, N=20, xs=i32(30, 40, 200, 100), ys=i32(3, 4, 200, 100), ss=i32(50, 60, 70, 80))
    c["two_keys_deep"] = dict(W=300, H=300, N=20, xs=i32(5, 12, 200, 100, 50, 25), ys=i32(3, 4, 200, 100, 50, 25), ss=i32(50, 60, 70, 80, 90, 95))
    # equal scores inside a node: the first in list order wins; quota 4 stops after the first pass, four keys share each node
    xs = i32(10, 20, 30, 40, 200, 210, 220, 230, 10, 20, 30, 40, 200, 210, 220, 230)
    ys = i32(10, 20, 30, 40, 10, 20, 30, 40, 200, 210, 220, 230, 200, 210, 220, 230)
    c["equal_scores"] = dict(W=300, H=300, N=4, xs=xs, ys=ys, ss=np.full(16, 80, np.int32))
    # the ORBextractor.cc:661 quirk: every multi-key node has all its keys in one quadrant, the pass leaves the size unchanged and ends the loop
    c["quirk_one_quadrant"] = dict(W=300, H=300, N=20, xs=i32(5, 9, 14, 200), ys=i32(5, 9, 14, 200), ss=i32(40, 90, 60, 70))
    # nIni 2..4 with an empty root (root compaction; the root's order parity is not a quadrant digit's)
    for n_ini, (W, H) in ((2, (500, 250)), (3, (600, 200)), (4, (640, 160))):
        rng = np.random.RandomState(77 + n_ini)
        hx = W // n_ini
        roots = [r for r in range(n_ini) if r != (1 if n_ini > 2 else 0)]
        r = rng.choice(roots, 120)
        x, y = r * hx + rng.randint(2, hx - 2, 120), rng.randint(0, H, 120)
        _, first = np.unique(y * 4096 + x, return_index=True); first.sort()
        c["empty_root_nini%d" % n_ini] = dict(W=W, H=H, N=40 if n_ini == 2 else 60, xs=x[first].astype(np.int32), ys=y[first].astype(np.int32),
                                              ss=rng.randint(7, 256, len(first)).astype(np.int32))
    c["quota_exact_full_pass"] = _search(300, 300, 16, 400, lambda i: not i["final"] and not i["quirk"] and i["T"] == 2)
    c["quota_mid_final"] = _search(300, 300, 40, 200, lambda i: i["final"] and i["mid_stop"])
    c["final_tie"] = _search(300, 300, 30, 90, lambda i: i["final"] and i["tie"] and i["mid_stop"])
    c["final_two_iterations"] = _search(300, 300, 12, 40, lambda i: i["final_iters"] >= 2 and i["depth"] <= 3, side=100)
    # a tight 20 x 20 block of 300 keys among 60 scattered ones (alone it would be one node after the first pass: all in one quadrant), across a
    # corner of the 31 x 32 FAST cells so that no cell list overflows: deeper than any table
    for seed in range(200):
        rng = np.random.RandomState(900 + seed)
        pick = np.sort(rng.permutation(400)[:300])
        bx, by = rng.randint(0, 588), rng.randint(0, 428)
        x = np.concatenate([rng.randint(0, 608, 60), bx + pick % 20]); y = np.concatenate([rng.randint(0, 448, 60), by + pick // 20])
        _, first = np.unique(y * 4096 + x, return_index=True); first.sort()
        x, y = x[first], y[first]
        sc = rng.randint(7, 256, len(x))
        info = {}
        octree_table(x, y, sc, 16, 16 + 608, 16, 16 + 448, 400, info=info)
        if info["depth"] >= 8 and np.bincount((y // 32) * 20 + x // 31).max() <= 200:
            break
    else:
        raise AssertionError("no seed gives a deep tight block")
    c["tight_block_deep"] = dict(W=608, H=448, N=400, xs=x.astype(np.int32), ys=y.astype(np.int32), ss=sc.astype(np.int32))
    # more than 2048 candidates (the kernel's global-memory key path)
    rng = np.random.RandomState(5)
    x, y = rng.randint(0, 608, 3200), rng.randint(0, 448, 3200)
    _, first = np.unique(y * 4096 + x, return_index=True); first.sort()
    assert len(first) > 2600
    c["many_keys"] = dict(W=608, H=448, N=400, xs=x[first].astype(np.int32), ys=y[first].astype(np.int32),
                          ss=rng.randint(7, 256, len(first)).astype(np.int32))
    return c


def block_image(w, h, seed, blocks):
    """Image whose FAST candidates crowd: random squares on a flat 128 background.  blocks = [(y0, y1, x0, x1, side), ...]: that rectangle is
    filled with side x side squares of uniform random grey; a later block overwrites an earlier one."""
    rng = np.random.RandomState(seed)
    img = np.full((h, w), 128, np.uint8)
    for y0, y1, x0, x1, side in blocks:
        ny, nx = -(-(y1 - y0) // side), -(-(x1 - x0) // side)
        tex = rng.randint(0, 256, (ny, nx)).astype(np.uint8).repeat(side, 0).repeat(side, 1)
        img[y0:y1, x0:x1] = tex[:y1 - y0, :x1 - x0]
    return img
