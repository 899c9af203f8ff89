"""The list builder shared by the two pose-graph optimisers (csrc/pose_graph_lists.h) in a stand-alone host program under the address
and undefined-behaviour sanitizers: free numbering, active edges, per block and per free vertex the contributions in edge order, at 7
and at 4 unknowns per vertex.  The free numbering and the active edges are compared with the numpy models' prepare(); the models sum
into a dense H and hold no block lists, so those are compared with a restatement here.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import essential_graph4dof_model as m4
import essential_graph_model as m7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-slam3-mac_amd", "csrc")

# vertices 0, 1 fixed; 2, 3, 4, 5 free (free indices 0..3); 5 has no edge: a diagonal block without items
FIXED = [1, 1, 0, 0, 0, 0]
EDGES = [(0, 1),      # both ends fixed: dropped
         (0, 2),      # one fixed end (side i)
         (2, 3),      # a free pair given as (low, high): kind 2, the transposed Ji^T Jj
         (4, 3),      # a free pair given as (high, low): kind 1
         (2, 3),      # the same pair again: one block, a second item
         (3, 2),      # and reversed: the same block, kind 1
         (4, 1)]      # one fixed end (side j)

MAIN = r"""
#include "pose_graph_lists.h"
#include <cstdio>
static void line(const char *name, const std::vector<int32_t> &v) { printf("%s", name); for (int32_t x : v) printf(" %d", (int)x); printf("\n"); }
int main()
{
    const uint8_t fixed[] = {FIXED};
    const int32_t v0[] = {V0}, v1[] = {V1};
    const int nv = sizeof(fixed), ne = sizeof(v0) / sizeof(v0[0]);
    const int dofs[2] = {7, 4}, strides[2] = {8, 12};
    for (int t = 0; t < 2; t++) {
        std::vector<double> meas((size_t)ne * strides[t]);
        for (size_t i = 0; i < meas.size(); i++) meas[i] = 1000.0 * (double)(i / strides[t]) + (double)(i % strides[t]);     // edge * 1000 + k
        PgLists H;
        pg_build_lists(nv, fixed, ne, v0, v1, meas.data(), dofs[t], strides[t], H);
        printf("graph dof %d nv %d ne %d nf %d n %d nblk %d\n", dofs[t], H.nv, H.ne, H.nf, H.n, H.nblk);
        line("free_idx", H.free_idx); line("free_list", H.free_list); line("v0", H.v0); line("v1", H.v1);
        line("blk_bi", H.blk_bi); line("blk_bj", H.blk_bj); line("blk_start", H.blk_start); line("blk_item", H.blk_item);
        line("vb_start", H.vb_start); line("vb_item", H.vb_item);
        printf("meas");
        for (double m : H.meas) printf(" %.0f", m);
        printf("\n");
    }
    PgLists E;                                          // no vertices, no edges
    pg_build_lists(0, fixed, 0, v0, v1, nullptr, 7, 8, E);
    printf("empty nf %d ne %d nblk %d starts %d %d\n", E.nf, E.ne, E.nblk, (int)E.blk_start.size(), (int)E.vb_start.size());
    return 0;
}
"""


def restated_lists(fixed, v0, v1):
    """Blocks: every diagonal one, then the off-diagonal ones in order of first appearance; items in edge order."""
    free = [i for i, f in enumerate(fixed) if not f]
    fidx = {v: k for k, v in enumerate(free)}
    act = [(a, b) for a, b in zip(v0, v1) if a in fidx or b in fidx]
    blocks, items, vb = [(f, f) for f in range(len(free))], [[] for _ in free], [[] for _ in free]
    for e, (a, b) in enumerate(act):
        fi, fj = fidx.get(a, -1), fidx.get(b, -1)
        if fi >= 0:
            items[fi].append(e << 2 | 0); vb[fi].append(e << 1 | 0)
        if fj >= 0:
            items[fj].append(e << 2 | 3); vb[fj].append(e << 1 | 1)
        if fi >= 0 and fj >= 0:
            key = (max(fi, fj), min(fi, fj))
            if key not in blocks:
                blocks.append(key); items.append([])
            items[blocks.index(key)].append(e << 2 | (1 if fi > fj else 2))
    return act, blocks, items, vb


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pg_lists")
    src, exe = tmp / "main.cc", str(tmp / "pg_lists")
    src.write_text(MAIN.replace("{FIXED}", "{%s}" % ", ".join(map(str, FIXED))).replace("{V0}", "{%s}" % ", ".join(str(a) for a, _ in EDGES))
                   .replace("{V1}", "{%s}" % ", ".join(str(b) for _, b in EDGES)))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "graph":
            cur = out.setdefault(int(w[2]), dict(zip(w[1::2], map(int, w[2::2]))))
        elif w[0] == "empty":
            out["empty"] = [int(x) for x in w[2::2][:3]] + [int(w[-2]), int(w[-1])]
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    return out


@pytest.mark.parametrize("dof,stride,model", [(7, 8, m7), (4, 12, m4)])
def test_lists_of_the_crafted_graph(printed, dof, stride, model):
    got = printed[dof]
    v0, v1 = [a for a, _ in EDGES], [b for _, b in EDGES]
    act, blocks, items, vb = restated_lists(FIXED, v0, v1)
    assert (got["nv"], got["ne"], got["nf"], got["n"], got["nblk"]) == (6, 6, 4, dof * 4, len(blocks))
    # free numbering and active edges: the numpy model's
    graph = dict(fixed=np.array(FIXED, np.uint8), edge_v0=np.array(v0, np.int32), edge_v1=np.array(v1, np.int32), edge_meas=np.zeros((len(EDGES), stride)))
    g = model.prepare(graph, False) if model is m7 else model.prepare(graph)
    assert got["free_idx"] == [int(x) for x in g["free_idx"]] and got["free_list"] == [2, 3, 4, 5]
    assert got["v0"] == [int(x) for x in g["a_v0"]] == [a for a, _ in act] and got["v1"] == [int(x) for x in g["a_v1"]] == [b for _, b in act]
    kept = [e for e in range(len(EDGES)) if bool(g["active"][e])]
    assert kept == [1, 2, 3, 4, 5, 6]
    assert got["meas"] == [1000 * e + k for e in kept for k in range(stride)]
    # blocks and items: the restatement, and the crafted graph's facts spelled out
    assert list(zip(got["blk_bi"], got["blk_bj"])) == blocks == [(0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (2, 1)]
    starts = np.concatenate([[0], np.cumsum([len(l) for l in items])]).tolist()
    assert got["blk_start"] == starts and got["blk_item"] == [x for l in items for x in l]
    per_blk = [got["blk_item"][got["blk_start"][k]:got["blk_start"][k + 1]] for k in range(got["nblk"])]
    assert per_blk[3] == []                                                    # the free vertex without edges
    assert per_blk[4] == [1 << 2 | 2, 3 << 2 | 2, 4 << 2 | 1]                   # (2,3) twice as (low, high), then (3,2): one block, edge order
    assert per_blk[5] == [2 << 2 | 1]                                           # (4,3) as (high, low)
    assert per_blk[0] == [0 << 2 | 3, 1 << 2 | 0, 3 << 2 | 0, 4 << 2 | 3]       # vertex 2: side j of (0,2), side i of (2,3) twice, side j of (3,2)
    vstarts = np.concatenate([[0], np.cumsum([len(l) for l in vb])]).tolist()
    assert got["vb_start"] == vstarts and got["vb_item"] == [x for l in vb for x in l]
    assert vb[2] == [2 << 1 | 0, 5 << 1 | 0] and vb[3] == []


def test_empty_graph(printed):
    assert printed["empty"] == [0, 0, 0, 1, 1]
