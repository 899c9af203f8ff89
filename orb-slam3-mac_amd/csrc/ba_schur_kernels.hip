// ba_schur_kernels.hip -- local bundle adjustment, the Schur complement S = Hpp + lambda I - W D^-1 W^T and bs = bp - W D^-1 bl (B6 of
// ba_kernels.hip's table, block_solver.hpp:354-438) in its three forms: the panel GEMM on the FP64 matrix cores (k_ba_schur_gemm +
// k_ba_schur_finish + k_ba_bschur), and from the device-built pair lists one 6x6 block pair per 16 or 64 lanes (k_ba_schur_big) or one
// row of blocks per workgroup (k_ba_schur_rows); k_ba_point_prep inverts the landmark blocks for all of them.  Last, the measured FP64
// MFMA peak the GEMM is judged against.  State and kernel argument: ba_batch.h; which form runs when: ba_kernels.hip.
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------------------------------------------- pair lists, built on the device
// The lists k_ba_schur_big / k_ba_schur_rows walk -- per graph and pair of free poses (i <= j, row-major over the upper triangle) the Hpl
// blocks of the points both see, in point order -- come from the pose-major edge lists that are uploaded anyway: a wave owns a pair, runs
// over pose i's edges 64 at a time (they are in point order) and finds each point among pose j's by a lower bound (the first edge of a
// (point, pose) chain is the one that carries the block).  Same entries in the same order as the host enumeration of round 3/4 -- every
// summation order downstream is unchanged -- without the 0.5 ms the host spent per 50 x 2000 x 10 window and the 2 MB it uploaded.
// FILL = 0: entries per pair into big_pair_start; k_ba_pair_scan turns them into starts; FILL = 1: the entries.
template <int FILL>
__global__ __launch_bounds__(256) void k_ba_pair_lists(BaBatch B)
{
    const BaGraphDev &G = B.gd[blockIdx.y];
    const int nf = G.nf, npair = nf * (nf + 1) / 2;
    const int lane = threadIdx.x & 63, pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= npair) return;
    int i = 0, j = pi;
    while (j >= nf - i) { j -= nf - i; i++; }
    j += i;
    const int *qs = B.pose_start + G.posestart_off, *pe = B.pose_edges + G.edge_off, *et = B.edge_task + G.edge_off, *ep = B.edge_point + G.edge_off;
    const int a0 = qs[i], a1 = qs[i + 1], c0 = qs[j], c1 = qs[j + 1];
    int *pstart = const_cast<int *>(B.big_pair_start) + G.pair_off;
    int2 *ent = const_cast<int2 *>(B.big_pair_ent) + G.pent_off, *jr = const_cast<int2 *>(B.big_pair_jr) + G.pent_off;
    int *ptl = const_cast<int *>(B.big_pair_pt) + G.pent_off;
    int out = FILL ? pstart[pi] : 0, rank = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int p0 = a0; p0 < a1; p0 += 64) {
        const int p = p0 + lane;
        int ta = -1, pt = -1;
        if (p < a1) { const int ea = pe[p]; ta = et[ea]; pt = ep[ea]; }
        const unsigned long long bb = __ballot(ta >= 0);
        const int myrank = rank + __popcll(bb & lt);             // place of the block in pose i's own (diagonal) list
        rank += __popcll(bb);
        int tc = -1;
        if (ta >= 0) {
            if (i == j) tc = ta;
            else {
                int lo = c0, hi = c1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (ep[pe[mid]] < pt) lo = mid + 1; else hi = mid; }
                if (lo < c1) { const int ec = pe[lo]; if (ep[ec] == pt) tc = et[ec]; }
            }
        }
        const unsigned long long hb = __ballot(tc >= 0);
        if (FILL && tc >= 0) {
            const int q = out + __popcll(hb & lt);
            ent[q] = make_int2(ta, tc); ptl[q] = pt; jr[q] = make_int2(tc, myrank);
        }
        out += __popcll(hb);
    }
    if (!FILL && lane == 0) pstart[pi] = out;
}
template __global__ void k_ba_pair_lists<0>(BaBatch);
template __global__ void k_ba_pair_lists<1>(BaBatch);
// counts -> exclusive starts, one workgroup per graph; entry npair = the graph's total
__global__ __launch_bounds__(256) void k_ba_pair_scan(BaBatch B)
{
    const BaGraphDev &G = B.gd[blockIdx.x];
    const int npair = G.nf * (G.nf + 1) / 2;
    int *ps = const_cast<int *>(B.big_pair_start) + G.pair_off;
    __shared__ int part[256];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int k0 = 0; k0 <= npair; k0 += 256) {
        const int k = k0 + threadIdx.x;
        const int v = k < npair ? ps[k] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        const int base = carry;
        if (k <= npair) ps[k] = base + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry = base + part[255];
        __syncthreads();
    }
}

// per trial: D = Hll + lambda I, D^-1 (symmetric), db = D^-1 bl   (block_solver.hpp:395-404)
__global__ __launch_bounds__(256) void k_ba_point_prep(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= G.n_points) return;
    const int *ps = B.pt_start + G.ptstart_off;
    double *Di = B.Dinv + (size_t)(G.point_off + l) * 6, *db = B.db + (size_t)(G.point_off + l) * 3;
    if (ps[l + 1] == ps[l]) { for (int i = 0; i < 6; i++) { Di[i] = 0; B.Linv[(size_t)(G.point_off + l) * 6 + i] = 0; } db[0] = db[1] = db[2] = 0; return; }
    const double *H = B.Hll + (size_t)(G.point_off + l) * 6;
    const double a00 = H[0] + st.lambda, a01 = H[1], a02 = H[2], a11 = H[3] + st.lambda, a12 = H[4], a22 = H[5] + st.lambda;
    const double c0 = a11 * a22 - a12 * a12, c1 = a12 * a02 - a01 * a22, c2 = a01 * a12 - a11 * a02;
    const double id = 1.0 / (a00 * c0 + a01 * c1 + a02 * c2);
    const double i00 = c0 * id, i01 = c1 * id, i02 = c2 * id;
    const double i11 = (a00 * a22 - a02 * a02) * id, i12 = (a02 * a01 - a00 * a12) * id, i22 = (a00 * a11 - a01 * a01) * id;
    Di[0] = i00; Di[1] = i01; Di[2] = i02; Di[3] = i11; Di[4] = i12; Di[5] = i22;
    {   // D = C C^T (Cholesky), Linv = C^-1: the Schur GEMM multiplies Z = C^-1 W, so that W^T D^-1 W = Z^T Z
        const double c00 = sqrt(a00), l00 = 1.0 / c00;
        const double c10 = a01 * l00, c20 = a02 * l00;
        const double c11 = sqrt(a11 - c10 * c10), l11 = 1.0 / c11;
        const double c21 = (a12 - c20 * c10) * l11;
        const double c22 = sqrt(a22 - c20 * c20 - c21 * c21), l22 = 1.0 / c22;
        const double l10 = -c10 * l00 * l11, l21 = -c21 * l11 * l22, l20 = -(l21 * c10 + l22 * c20) * l00;
        double *Lo = B.Linv + (size_t)(G.point_off + l) * 6;
        Lo[0] = l00; Lo[1] = l10; Lo[2] = l11; Lo[3] = l20; Lo[4] = l21; Lo[5] = l22;
    }
    const double *b = B.bl + (size_t)(G.point_off + l) * 3;
    db[0] = i00 * b[0] + i01 * b[1] + i02 * b[2];
    db[1] = i01 * b[0] + i11 * b[1] + i12 * b[2];
    db[2] = i02 * b[0] + i12 * b[1] + i22 * b[2];
}

// Schur GEMM on the FP64 matrix cores:  S_sub = W^T D^-1 W = Z^T Z  with  Z = C^-1 W,  D = C C^T  (k_ba_point_prep), over the
// K-padded dense panel Z[4l+b][c] (K = 4 per point: 3 + pad), v_mfma_f64_16x16x4_f64:
//   A[i][k] (lane i=l&15,k=l>>4), B[k][j] (lane j=l&15,k=l>>4), C/D 4 regs: col = l&15, row = (l>>4) + 4*reg.
// One 512-thread workgroup (8 waves, up to 256 VGPRs each) owns a range of STAGES (<= GEMM_PS points, <= GEMM_STAGE_EDGES Hpl
// blocks) of one graph.  The dense panel exists only in LDS: per stage every thread fetches ONE column of ONE sparse Hpl block
// (3 doubles of Wsp, loaded a stage ahead into registers), multiplies it by the point's C^-1 and scatters it into the cleared stage
// buffer -- HBM sees the 144-byte blocks (0.7 GB per 256 graphs) instead of a 79 %-zero dense panel (3.5 GB), and both MFMA
// fragments come straight from the same LDS panel (no D^-1 arithmetic between load and MFMA).  The upper 16x16 output tiles stay
// in accumulator registers for the whole launch.
// Tile ownership: every row strip of the upper triangle is cut into CHUNKS of GEMM_C consecutive tiles; chunk i belongs to wave
// i % 8, slot i / 8 (GEMM_NCH slots per wave).  Block sparsity: a point is seen by ~10 of ~48 free keyframes; which (point, chunk,
// tile) combinations of a stage hold data is decided once per stage by all 64 lanes (lane = 8*point + chunk) and three ballots;
// a hit chunk loads its A fragment and GEMM_C B fragments back to back and issues the MFMAs of its non-empty tiles.
// LDS rows are padded to ld+16 doubles so that the K-rows of a fragment fall into different bank halves.
// (GEMM_PS, GEMM_C, GEMM_NCH, GEMM_WAVES, GEMM_LDS_PAD, GEMM_STAGE_EDGES, GEMM_TARGET_WGS, GEMM_PANEL_LDS_BYTES and gemm_strip_chunks: ba_graph_lists.h,
// with the host code that cuts the stages by them; GEMM_LDS_TAIL: ba_batch.h, the host sizes the LDS by it)
static_assert(GEMM_PS * GEMM_NCH <= 64 && GEMM_NCH * GEMM_C <= 32, "one lane per (stage point, chunk); one valid bit per tile");
static_assert(6 * GEMM_STAGE_EDGES <= 64 * GEMM_WAVES && 6 * GEMM_PS <= 64 * GEMM_WAVES, "one column task per thread");
__global__ __launch_bounds__(64 * GEMM_WAVES) void k_ba_schur_gemm(BaBatch B)
{
    extern __shared__ double glds[];               // [2][gemm_ps][3][ld + pad] Z rows of the stage, double buffered (+ tail)
    __shared__ __attribute__((aligned(16))) double s_raw[2][GEMM_STAGE_EDGES * 18];   // the stage's Hpl blocks as they lie in Wsp
    __shared__ __attribute__((aligned(16))) int4 s_task[2][GEMM_STAGE_EDGES];
    __shared__ __attribute__((aligned(16))) double s_linv[2][GEMM_PS][6];
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[3][GEMM_PS];
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nt = G.nt16;
    if ((int)blockIdx.x >= G.ks * G.ngrp) return;
    const int ksi = blockIdx.x / G.ngrp, grp = blockIdx.x - ksi * G.ngrp;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const int ld = G.ld, ldp = ld + GEMM_LDS_PAD;
    // this wave's chunks: offsets of the row tile / first column tile inside an LDS row (wave-uniform -> scalar registers)
    int aoff[GEMM_NCH], boffc[GEMM_NCH];
    uint32_t cvalid = 0;                                 // tiles that exist: bit c*GEMM_C + j
    v4d acc[GEMM_NCH * GEMM_C];
#pragma unroll
    for (int c = 0; c < GEMM_NCH; c++) {
        int id = (grp * GEMM_NCH + c) * GEMM_WAVES + wv, tr = 0;
        while (tr < nt && id >= gemm_strip_chunks(nt, tr)) { id -= gemm_strip_chunks(nt, tr); tr++; }
        if (tr < nt) {
            const int tc = tr + id * GEMM_C, len = min(GEMM_C, nt - tc);
            aoff[c] = 16 * tr; boffc[c] = 16 * tc; cvalid |= ((1u << len) - 1u) << (c * GEMM_C);
        } else { aoff[c] = 0; boffc[c] = 0; }
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) acc[c * GEMM_C + j] = (v4d){0, 0, 0, 0};
    }
    // the same table per LANE for the once-per-stage hit evaluation: lane = 8*point + chunk decides (point, chunk) for all
    // GEMM_PS x GEMM_NCH = 64 combinations at once; the ballots replace ~20 scalar instructions per (point, chunk)
    uint32_t lrow = 0, lcolbit[GEMM_C];
    {
        const int c = lane % GEMM_NCH;
        int id = (grp * GEMM_NCH + c) * GEMM_WAVES + wv, tr = 0;
        while (tr < nt && id >= gemm_strip_chunks(nt, tr)) { id -= gemm_strip_chunks(nt, tr); tr++; }
        const int tc = tr + id * GEMM_C;
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) lcolbit[j] = (tr < nt && tc + j < nt) ? 1u << (tc + j) : 0u;
        if (tr < nt) lrow = 1u << tr;
    }
    const int per = (G.n_stages + G.ks - 1) / G.ks;
    const int sb = ksi * per, se = min(G.n_stages, sb + per);
    const int4 *stg = B.gemm_stage + G.stage_off;          // {first point, points, first task, tasks}
    const int4 *tsk = B.gemm_task + G.gemm_off;            // {edge, 6*h, point, -}
    const double live = lk < 3 ? 1.0 : 0.0;                // K-row 3 is the pad: A is zero there, B re-reads row 2 (finite)
    const int boff = min(lk, 2) * ldp + li;
    const size_t stage_doubles = (size_t)G.gemm_ps * 3 * ldp;
    // stage s -> LDS by asynchronous global -> LDS copies (no staging registers): its Hpl blocks (contiguous in Wsp), task
    // descriptors, C^-1 rows and occupancy masks; issued two stages ahead of the multiply
    auto dma16 = [&](const void *src, void *dst, int bytes) {          // wave-strided 1-KiB pieces, 16 B per lane
        for (int piece = wv; piece * 1024 < bytes; piece += GEMM_WAVES)
            if (piece * 1024 + lane * 16 < bytes)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)src + piece * 1024 + lane * 16),
                                                 (__attribute__((address_space(3))) void *)((char *)dst + piece * 1024), 16, 0, 0);
    };
    auto load_stage = [&](int s) {
        const int4 sd = stg[s];
        const int b2 = s & 1;
        dma16(B.Wsp + (size_t)(G.gemm_off + sd.z) * 18, &s_raw[b2][0], sd.w * 144);
        dma16(tsk + sd.z, &s_task[b2][0], sd.w * 16);
        if (wv == 0) {
            if (lane * 16 < sd.y * 48)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)(B.Linv + (size_t)(G.point_off + sd.x) * 6) + lane * 16),
                                                 (__attribute__((address_space(3))) void *)&s_linv[b2][0][0], 16, 0, 0);
        } else if (wv == 1) {
            if (lane < sd.y)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(B.ptmask + G.point_off + sd.x + lane),
                                                 (__attribute__((address_space(3))) void *)&s_mask[s % 3][0], 4, 0, 0);
        }
    };
    auto clear = [&](int buf) {                            // the stage buffer starts from zero
        double2 *z = reinterpret_cast<double2 *>(glds + buf * stage_doubles);
        for (int i = tid; i < (int)(stage_doubles / 2); i += 64 * GEMM_WAVES) z[i] = make_double2(0.0, 0.0);
    };
    auto scatter = [&](int s, int buf) {                   // Z = C^-1 W, one column of one block per thread
        const int b2 = s & 1, ntask = stg[s].w, pt0 = stg[s].x;
        if (tid < 6 * ntask) {
            const int i = tid / 6, a = tid - 6 * i;
            const int4 t = s_task[b2][i];
            const double *w = &s_raw[b2][18 * i + a];
            const double w0 = w[0], w1 = w[6], w2 = w[12];
            const int wp = t.z - pt0;
            const double *L = s_linv[b2][wp];
            double *dst = glds + buf * stage_doubles + (size_t)wp * 3 * ldp + t.y + a;
            dst[0] = L[0] * w0;
            dst[ldp] = L[1] * w0 + L[2] * w1;
            dst[2 * ldp] = L[3] * w0 + L[4] * w1 + L[5] * w2;
        }
    };
    if (sb < se) {
        load_stage(sb);
        if (sb + 1 < se) load_stage(sb + 1);
        clear(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        scatter(sb, 0);
    }
    int cur = 0;
    for (int s = sb; s < se; s++, cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's copies of stage s+1 have landed
        __syncthreads();                                    // stage s is scattered; everyone is done with the other buffer and has its copies
        if (s + 1 < se) clear(cur ^ 1);
        __syncthreads();
        if (s + 1 < se) { scatter(s + 1, cur ^ 1); }
        if (s + 2 < se) load_stage(s + 2);                  // reuses the raw / task / C^-1 slots of stage s (scattered one iteration ago)
        const int np = stg[s].y;
        const double *stage = glds + cur * stage_doubles;
        // which (point, chunk, tile) combinations of this stage hold data: one evaluation per lane, GEMM_C ballots
        unsigned long long hit[GEMM_C];
        {
            const int pl = lane / GEMM_NCH;
            const uint32_t m = pl < np ? s_mask[s % 3][pl] : 0u;
            const bool rh = (m & lrow) != 0;
#pragma unroll
            for (int j = 0; j < GEMM_C; j++) hit[j] = __ballot(rh && (m & lcolbit[j]));
        }
        for (int p = 0; p < np; p++) {
            uint32_t tj[GEMM_C], any = 0;
#pragma unroll
            for (int j = 0; j < GEMM_C; j++) { tj[j] = (uint32_t)(hit[j] >> (GEMM_NCH * p)) & ((1u << GEMM_NCH) - 1u); any |= tj[j]; }
            if (any == 0) continue;                         // the point touches none of this wave's chunks
            const double *rows = stage + (size_t)p * 3 * ldp + boff;
#pragma unroll
            for (int c = 0; c < GEMM_NCH; c++) {
                if (any & (1u << c)) {
                    const double az = rows[aoff[c]];
                    double bf[GEMM_C];
#pragma unroll
                    for (int j = 0; j < GEMM_C; j++) bf[j] = rows[boffc[c] + 16 * j];   // tiles past nt: pad garbage, never multiplied
                    __builtin_amdgcn_sched_barrier(0);          // all 1 + GEMM_C LDS reads in flight before the first wait
                    const double a = live * az;
#pragma unroll
                    for (int j = 0; j < GEMM_C; j++)
                        if (tj[j] & (1u << c))                  // the fragments are already in registers: an empty tile costs one scalar test
                            acc[c * GEMM_C + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bf[j], acc[c * GEMM_C + j], 0, 0, 0);
                }
            }
        }
    }
    double *Sp = B.Spart + G.spart_off + (size_t)ksi * ld * ld;
#pragma unroll
    for (int c = 0; c < GEMM_NCH; c++) {
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) {
            if ((cvalid >> (c * GEMM_C + j)) & 1u) {
#pragma unroll
                for (int r = 0; r < 4; r++) Sp[(size_t)(aoff[c] + lk + 4 * r) * ld + boffc[c] + 16 * j + li] = acc[c * GEMM_C + j][r];
            }
        }
    }
}

// S = blockdiag(Hpp + lambda I) - sum_ks Spart (mirrored from the upper tiles); padding rows -> identity
__global__ __launch_bounds__(256) void k_ba_schur_finish(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.ld * G.ld) return;
    const int r = idx / G.ld, c = idx - r * G.ld;
    double v = 0;
    if (r >= G.n || c >= G.n) v = (r == c) ? 1.0 : 0.0;
    else {
        if (r / 6 == c / 6) v = B.Hpp[(size_t)(G.free_off + r / 6) * 36 + (r % 6) * 6 + (c % 6)] + (r == c ? st.lambda : 0.0);
        const int ur = (r / 16 <= c / 16) ? r : c, uc = (r / 16 <= c / 16) ? c : r;   // upper-tile source
        double s = 0;
        if (B.world == 1) {
            const double *Sp = B.Spart + G.spart_off + (size_t)ur * G.ld + uc;
            for (int k = 0; k < G.ks; k++) s += Sp[(size_t)k * G.ld * G.ld];
        } else {
            const double *X = B.xbuf + B.x2_off[g] + (size_t)ur * G.ld + uc;          // every rank's sum_ks Spart, rank order
            for (int r = 0; r < B.world; r++) s += X[(size_t)r * B.xcount];
        }
        v -= s;
    }
    B.S[G.s_off + idx] = v;
}

// bs = bp - sum_{edges of pose} W_e * db_point   (block_solver.hpp:409-416,435-438), one wave per free pose
__global__ __launch_bounds__(64) void k_ba_bschur(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int h = blockIdx.x;
    if (h >= G.nf) return;
    const int lane = threadIdx.x;
    const int *qs = B.pose_start + G.posestart_off;
    const int *pe = B.pose_edges + G.edge_off;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = qs[h] + lane; k < qs[h + 1]; k += 64) {
        const int task = B.pm_task[(size_t)G.edge_off + k];                // pose-major copies: only the block and db are gathers
        if (task < 0) continue;                                            // one Hpl block per (point, pose)
        const int l = B.pm_point[(size_t)G.edge_off + k];
        const double *db = B.db + (size_t)(G.point_off + l) * 3;
        const double *w = B.Wsp + (size_t)task * 18;
        for (int a = 0; a < 6; a++) acc[a] += w[a] * db[0] + w[6 + a] * db[1] + w[12 + a] * db[2];
    }
    for (int a = 0; a < 6; a++) {
        double v = acc[a];
        v = wave_sum_f64_dpp(v);
        acc[a] = v;
    }
    if (lane == 0)
        for (int a = 0; a < 6; a++) {
            B.bacc[(size_t)(G.free_off + h) * 6 + a] = acc[a];
            B.bs[(size_t)(G.free_off + h) * 6 + a] = B.bp[(size_t)(G.free_off + h) * 6 + a] - acc[a];      // sharded: redone by k_ba_shard_sum2
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// Windows with more than 80 free keyframes (n = 6 nf > BA_LDLT_MAXN; the reference has no cap: Optimizer.cc:1703-1819 takes
// every covisible keyframe, the merge variant :6255 two whole neighbourhoods), and smaller ones where the pair form is chosen:
//   k_ba_schur_big      S_ij = sum over the points seen by free poses i and j of W_i D^-1 W_j^T, one wave per 6x6 block pair,
//                       fixed summation order (block_solver.hpp:381-432 restated per output block)
// (the factorisation of such a window: ba_reduced_kernels.hip)
// LPP = lanes per pair: 16 (four pairs per wave; batches) or 64 (one pair per wave: with a handful of windows the chip is empty and the
// per-pair chain -- entries / lanes dependent gather rounds -- is what a tick waits for)
template <int LPP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ba_schur_big(BaBatch B, int nblk)
{
    constexpr int PPW = 64 / LPP;                                  // pairs per wave
    // FOUR block pairs per wave, 16 lanes each: the 36 sums of a pair are reduced inside its 16-lane DPP row (4 rotate-add steps
    // instead of 6 scan steps + a readlane over the wave) and four pairs share the issue slots -- 2.6x fewer instructions per pair
    // than one wave per pair, which made this kernel faster than the MFMA panel GEMM for every batch size.
    // blockIdx -> (graph, block of 4 pairs): all blocks of a graph run on ONE XCD (workgroups are dealt round-robin over the 8 XCDs), one
    // graph after the other per XCD, so that the graph's Hpl blocks (2.9 MB at 50 x 2000 x 10; every block is read ~11 times, once per
    // pair it belongs to) stay in that XCD's 4 MB L2 instead of being fetched again from HBM
    int g, blk;
    if (B.G >= 8) { const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3; g = xcd + 8 * (slot / nblk); blk = slot - (slot / nblk) * nblk; }
    else { g = blockIdx.x / nblk; blk = blockIdx.x - g * nblk; }               // few graphs: every graph over the whole chip
    if (g >= B.G) return;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nf = G.nf;
    const int lane = threadIdx.x, sub = lane & (LPP - 1);
    const int pair = blk * PPW + lane / LPP;
    if (pair >= nf * (nf + 1) / 2) return;                          // whole rows leave together (row-local DPP below)
    int i = 0, bp = pair;
    while (bp >= nf - i) { bp -= nf - i; i++; }
    const int j = i + bp;
    const int *ps = B.big_pair_start + G.pair_off + pair;
    const int2 *ent = B.big_pair_ent + G.pent_off;
    const int *entl = B.big_pair_pt + G.pent_off;
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0.0;
    // the list entry (two block indices + point) of the NEXT trip is fetched a trip ahead: index load and block gathers are two dependent
    // L2 round trips, this takes the first one off the chain
    const int e_end = ps[1];
    int en = ps[0] + sub;
    int2 tn = make_int2(0, 0); int ln = 0;
    if (en < e_end) { tn = ent[en]; ln = entl[en]; }
    for (int e = en; e < e_end; e += LPP) {
        const int2 t = tn;
        const int l = ln;
        if (e + LPP < e_end) { tn = ent[e + LPP]; ln = entl[e + LPP]; }
        const double *Di = B.Dinv + (size_t)(G.point_off + l) * 6;       // (Hll + lambda I)^-1, upper triangle
        const double i00 = Di[0], i01 = Di[1], i02 = Di[2], i11 = Di[3], i12 = Di[4], i22 = Di[5];
        const double *wa = B.Wsp + (size_t)t.x * 18, *wb = B.Wsp + (size_t)t.y * 18;
        double y0[6], y1[6], y2[6];                                     // Y = W_a D^-1 (block_solver.hpp:398-407), then acc += Y W_b^T
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double a0 = wa[a], a1 = wa[6 + a], a2 = wa[12 + a];
            y0[a] = a0 * i00 + a1 * i01 + a2 * i02;
            y1[a] = a0 * i01 + a1 * i11 + a2 * i12;
            y2[a] = a0 * i02 + a1 * i12 + a2 * i22;
        }
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double b0 = wb[c], b1 = wb[6 + c], b2 = wb[12 + c];
#pragma unroll
            for (int r = 0; r < 6; r++) acc[6 * r + c] += y0[r] * b0 + y1[r] * b1 + y2[r] * b2;
        }
    }
    // the finished block goes straight into S = blockdiag(Hpp + lambda I) - sum, both triangles (no partial-sum buffer, no finish
    // kernel on this path; rows / columns >= n of the padded matrix are never read by the factorisations)
    double *S = B.S + G.s_off;
    const double lambda = st.lambda;
    const double *Hd = B.Hpp + (size_t)(G.free_off + i) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) {
        const double v = LPP == 16 ? row16_allreduce_f64_dpp(acc[k]) : wave_sum_f64_dpp(acc[k]);      // every lane of the group holds the sum
        if (sub == 0) {
            const int r = k / 6, c = k - 6 * r;
            const double out = (i == j ? Hd[k] + (r == c ? lambda : 0.0) : 0.0) - v;
            S[(size_t)(6 * i + r) * G.ld + 6 * j + c] = out;
            if (i != j) S[(size_t)(6 * j + c) * G.ld + 6 * i + r] = out;
        }
    }
    // bs = bp - W D^-1 b_l (block_solver.hpp:409-416, 435-438): the diagonal pair lists every Hpl block of pose i exactly once; a second,
    // short pass over it (its blocks are in L2 now) -- inside the loop above the extra branch and registers cost more than they saved
    if (i == j) {
        double wdb[6] = {0, 0, 0, 0, 0, 0};
        for (int e = ps[0] + sub; e < ps[1]; e += LPP) {
            const double *w = B.Wsp + (size_t)ent[e].x * 18, *db = B.db + (size_t)(G.point_off + entl[e]) * 3;
            const double d0 = db[0], d1 = db[1], d2 = db[2];
#pragma unroll
            for (int a = 0; a < 6; a++) wdb[a] += w[a] * d0 + w[6 + a] * d1 + w[12 + a] * d2;
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double v = LPP == 16 ? row16_allreduce_f64_dpp(wdb[a]) : wave_sum_f64_dpp(wdb[a]);
            if (sub == 0) { B.bacc[(size_t)(G.free_off + i) * 6 + a] = v; B.bs[(size_t)(G.free_off + i) * 6 + a] = B.bp[(size_t)(G.free_off + i) * 6 + a] - v; }
        }
    }
}
template __global__ void k_ba_schur_big<16>(BaBatch, int);
template __global__ void k_ba_schur_big<64>(BaBatch, int);

// The same sums, one 256-thread workgroup per ROW i of the block matrix (round 3).  k_ba_schur_big gathers, per list entry, BOTH Hpl blocks
// and the point's D^-1 from L2: 5-6 cache lines for 162 multiply-adds, 9 GB per launch at 256 windows, and the gather path (one line per
// lane per load instruction) is what the kernel waits for.  All pairs (i, j >= i) share pose i's side: the workgroup computes
// Y_il = W_il D_l^-1 for every block of pose i ONCE into LDS (the diagonal pair's list enumerates them in point order; an entry carries
// the rank of its i-side block in that list), then its sixteen 16-lane groups take the pairs of the row round-robin and gather only W_jl:
// 2 lines per entry, a third of the multiply-adds gone.  Expressions and summation order are k_ba_schur_big<16>'s, so the two kernels
// agree bit for bit on every off-diagonal block (the diagonal blocks and bs are summed in another association, see below).  Rows are dealt
// like the pairs were: a graph's rows on one XCD, longest rows first.
// (SROW_THREADS, SROW_GROUPS, SROW_MAX_BLOCKS: ba_batch.h, the host sizes the launch and the LDS by them)
__global__ __launch_bounds__(SROW_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_ba_schur_rows(BaBatch B, int max_nf)
{
    extern __shared__ __attribute__((aligned(16))) double srow_y[];          // [blocks of pose i][18]: y0[6] y1[6] y2[6]
    __shared__ double s_part[SROW_GROUPS * 27];                              // the diagonal block's and W db's partial sums, one set per 16-lane group
    __shared__ int s_next;                                                   // next pair of the row nobody has taken
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int g = xcd + 8 * (slot / max_nf), i = slot - (slot / max_nf) * max_nf;
    if (g >= B.G) return;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nf = G.nf;
    if (i >= nf) return;
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const int *ps = B.big_pair_start + G.pair_off + (i * nf - i * (i - 1) / 2);      // pairs (i, i), (i, i + 1), ...
    const int2 *ent = B.big_pair_ent + G.pent_off;
    const int *entl = B.big_pair_pt + G.pent_off;
    const int2 *entjr = B.big_pair_jr + G.pent_off;
    if (tid == 0) s_next = i + 1 + SROW_GROUPS;
    // ---- pose i's own blocks, one per thread: Y into LDS, and the diagonal pair (i, i) on the way -- its list IS this enumeration, and as
    // one 16-lane group's chain (400 entries at 50 x 2000 x 10) it would outlast every other pair of the row by a factor of five while the
    // workgroup holds its LDS.  S_ii and bs = bp - W D^-1 b_l are summed per thread, per 16-lane group (DPP), then over the groups in order.
    {
        const int d0 = ps[0], nblk = ps[1] - d0;
        double dacc[21], wdb[6];                       // S_ii is symmetric: its lower triangle, row-major
#pragma unroll
        for (int k = 0; k < 21; k++) dacc[k] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) wdb[a] = 0.0;
        for (int p = tid; p < nblk; p += SROW_THREADS) {
            const int l = entl[d0 + p];
            const double *Di = B.Dinv + (size_t)(G.point_off + l) * 6, *db = B.db + (size_t)(G.point_off + l) * 3;
            const double i00 = Di[0], i01 = Di[1], i02 = Di[2], i11 = Di[3], i12 = Di[4], i22 = Di[5];
            const double d0b = db[0], d1b = db[1], d2b = db[2];
            const double2 *wa2 = reinterpret_cast<const double2 *>(B.Wsp + (size_t)ent[d0 + p].x * 18);       // 144-byte blocks: 16-byte aligned
            double wa[18], y0[6], y1[6], y2[6];
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 v = wa2[k]; wa[2 * k] = v.x; wa[2 * k + 1] = v.y; }
            double *y = srow_y + 18 * p;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double a0 = wa[a], a1 = wa[6 + a], a2 = wa[12 + a];
                y0[a] = a0 * i00 + a1 * i01 + a2 * i02;
                y1[a] = a0 * i01 + a1 * i11 + a2 * i12;
                y2[a] = a0 * i02 + a1 * i12 + a2 * i22;
                y[a] = y0[a]; y[6 + a] = y1[a]; y[12 + a] = y2[a];
                wdb[a] += a0 * d0b + a1 * d1b + a2 * d2b;
            }
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c <= r; c++) dacc[r * (r + 1) / 2 + c] += y0[r] * wa[c] + y1[r] * wa[6 + c] + y2[r] * wa[12 + c];
        }
#pragma unroll
        for (int k = 0; k < 21; k++) { const double v = row16_allreduce_f64_dpp(dacc[k]); if (sub == 0) s_part[27 * grp + k] = v; }
#pragma unroll
        for (int a = 0; a < 6; a++) { const double v = row16_allreduce_f64_dpp(wdb[a]); if (sub == 0) s_part[27 * grp + 21 + a] = v; }
    }
    __syncthreads();
    double *S = B.S + G.s_off;
    if (tid < 27) {
        double v = 0.0;
        for (int q = 0; q < SROW_GROUPS; q++) v += s_part[27 * q + tid];
        if (tid < 21) {
            int r = 0, c = tid;
            while (c > r) { c -= r + 1; r++; }
            const double out = B.Hpp[(size_t)(G.free_off + i) * 36 + 6 * r + c] + (r == c ? st.lambda : 0.0) - v;
            S[(size_t)(6 * i + r) * G.ld + 6 * i + c] = out;
            S[(size_t)(6 * i + c) * G.ld + 6 * i + r] = out;
        } else {
            const size_t o = (size_t)(G.free_off + i) * 6 + tid - 21;
            B.bacc[o] = v; B.bs[o] = B.bp[o] - v;
        }
    }
    // ---- the pairs (i, j > i), handed out dynamically (list lengths differ by an order of magnitude): the first one per group by index, then
    // from the counter
    for (int j = i + 1 + grp; j < nf; j = row16_allreduce_add_dpp(sub == 0 ? atomicAdd(&s_next, 1) : 0)) {
        const int e0 = ps[j - i], e_end = ps[j - i + 1];
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; k++) acc[k] = 0.0;
        const int en = e0 + sub;                                       // the NEXT trip's list entry is fetched a trip ahead
        int2 tn = make_int2(0, 0);
        if (en < e_end) tn = entjr[en];
        for (int e = en; e < e_end; e += 16) {
            const int bj = tn.x, pos = tn.y;
            if (e + 16 < e_end) tn = entjr[e + 16];
            const double2 *wb2 = reinterpret_cast<const double2 *>(B.Wsp + (size_t)bj * 18);
            double wb[18];
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 v = wb2[k]; wb[2 * k] = v.x; wb[2 * k + 1] = v.y; }
            const double *y = srow_y + 18 * pos;
            double y0[6], y1[6], y2[6];
#pragma unroll
            for (int a = 0; a < 6; a++) { y0[a] = y[a]; y1[a] = y[6 + a]; y2[a] = y[12 + a]; }
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const double b0 = wb[c], b1 = wb[6 + c], b2 = wb[12 + c];
#pragma unroll
                for (int r = 0; r < 6; r++) acc[6 * r + c] += y0[r] * b0 + y1[r] * b1 + y2[r] * b2;
            }
        }
#pragma unroll
        for (int k = 0; k < 36; k++) {
            const double v = row16_allreduce_f64_dpp(acc[k]);
            if (sub == 0) {
                const int r = k / 6, c = k - 6 * r;
                S[(size_t)(6 * i + r) * G.ld + 6 * j + c] = -v;
                S[(size_t)(6 * j + c) * G.ld + 6 * i + r] = -v;
            }
        }
    }
}

// FP64 matrix-core peak of this device, measured: every wave issues independent
// v_mfma_f64_16x16x4_f64 chains (the local micro-architecture guide lists no FP64 MFMA peak).
__global__ __launch_bounds__(256) void k_mfma_f64_peak(double *sink, int iters)
{
    v4d acc[8];
    for (int i = 0; i < 8; i++) acc[i] = (v4d){0, 0, 0, 0};
    const double a = 1.0 + threadIdx.x * 1e-9, bb = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; it++)
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[i], 0, 0, 0);
    double s = 0;
    for (int i = 0; i < 8; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[0] = s;
}

extern "C" int orbhip_mfma_f64_peak_tflops(orbhip_ctx *ctx, double *tflops_out)
{
    if (!ctx || !tflops_out) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    double *sink = nullptr;
    if (hipMalloc((void **)&sink, 8) != hipSuccess) return ORBHIP_E_HIP;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int blocks = 256 * 8, iters = 4096;
    hipLaunchKernelGGL(k_mfma_f64_peak, dim3(blocks), dim3(256), 0, s, sink, 64);          // warm-up
    (void)hipEventRecord(e0, s);
    hipLaunchKernelGGL(k_mfma_f64_peak, dim3(blocks), dim3(256), 0, s, sink, iters);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(sink);
    const double flops = (double)blocks * 4.0 * iters * 8.0 * 2048.0;
    *tflops_out = flops / (ms * 1e-3) / 1e12;
    return ORBHIP_OK;
}
