// pose_graph_lists.h -- the host's lists of one pose graph, built once per call and shared by the Sim3 graph (pose_graph_kernels.hip,
// 7 unknowns per vertex) and the 4-DoF graph (pose_graph4dof_kernels.hip): free numbering in ABI order, active edges in edge order,
// per block of the lower block triangle of H and per free vertex the contributions in edge order.  k_pg*_assemble sums in exactly
// these orders, so they are part of the result's bits.  Nothing from HIP is included: a host compiler builds this header alone
// (tests/test_pose_graph_lists.py does, under the address and undefined-behaviour sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

struct PgLists {
    int nv = 0, ne = 0, nf = 0, n = 0, nblk = 0;     // vertices, ACTIVE edges, free vertices, unknowns, blocks
    std::vector<int32_t> free_idx, free_list;        // [nv] -> free index or -1; [nf] -> vertex
    std::vector<int32_t> v0, v1;                     // [ne]
    std::vector<int32_t> blk_bi, blk_bj, blk_start, blk_item;    // block (bi >= bj); items: edge << 2 | kind (0 Ji^T Ji, 1 Ji^T Jj, 2 its transpose, 3 Jj^T Jj)
    std::vector<int32_t> vb_start, vb_item;          // per free vertex; items: edge << 1 | side
    std::vector<double> meas;                        // [ne][meas_stride]
};

// dof: unknowns per vertex; meas_stride: doubles per edge of edge_meas
inline void pg_build_lists(int n_vertices, const uint8_t *fixed, int n_edges, const int32_t *edge_v0, const int32_t *edge_v1, const double *edge_meas,
                           int dof, int meas_stride, PgLists &H)
{
    H.nv = n_vertices;
    H.free_idx.assign(H.nv, -1);
    for (int v = 0; v < H.nv; v++) if (!fixed[v]) { H.free_idx[v] = (int32_t)H.free_list.size(); H.free_list.push_back(v); }
    H.nf = (int)H.free_list.size(); H.n = dof * H.nf;
    for (int e = 0; e < n_edges; e++) {
        const int a = edge_v0[e], b = edge_v1[e];
        if (H.free_idx[a] < 0 && H.free_idx[b] < 0) continue;                // not active (sparse_optimizer.cpp:234)
        H.v0.push_back(a); H.v1.push_back(b);
        for (int k = 0; k < meas_stride; k++) H.meas.push_back(edge_meas[meas_stride * (size_t)e + k]);
    }
    H.ne = (int)H.v0.size();
    // blocks: every diagonal block, then the off-diagonal ones in order of first appearance
    std::map<std::pair<int, int>, int> id;
    std::vector<std::vector<int32_t>> items(H.nf), vb(H.nf);
    for (int f = 0; f < H.nf; f++) { id[{f, f}] = f; H.blk_bi.push_back(f); H.blk_bj.push_back(f); }
    for (int e = 0; e < H.ne; e++) {
        const int fi = H.free_idx[H.v0[e]], fj = H.free_idx[H.v1[e]];
        if (fi >= 0) { items[fi].push_back(e << 2 | 0); vb[fi].push_back(e << 1 | 0); }
        if (fj >= 0) { items[fj].push_back(e << 2 | 3); vb[fj].push_back(e << 1 | 1); }
        if (fi >= 0 && fj >= 0) {
            const std::pair<int, int> key = fi > fj ? std::make_pair(fi, fj) : std::make_pair(fj, fi);
            auto it = id.find(key);
            if (it == id.end()) { it = id.emplace(key, (int)items.size()).first; items.emplace_back(); H.blk_bi.push_back(key.first); H.blk_bj.push_back(key.second); }
            items[it->second].push_back(e << 2 | (fi > fj ? 1 : 2));         // Ji^T (W) Jj is block (fi, fj); below the diagonal as it is, else transposed
        }
    }
    H.nblk = (int)items.size();
    H.blk_start.push_back(0);
    for (auto &l : items) { H.blk_item.insert(H.blk_item.end(), l.begin(), l.end()); H.blk_start.push_back((int32_t)H.blk_item.size()); }
    H.vb_start.push_back(0);
    for (auto &l : vb) { H.vb_item.insert(H.vb_item.end(), l.begin(), l.end()); H.vb_start.push_back((int32_t)H.vb_item.size()); }
}
