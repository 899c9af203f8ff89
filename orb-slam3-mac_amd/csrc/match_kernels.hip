// match_kernels.hip -- the windowed searches for projected map points (reference src/ORBmatcher.cc): SearchByProjection against the
// last frame (:1965-2181) and the local map (:48-218), sequential and replay form, and the search part of Fuse (:1403-1613).  All of
// them walk the Frame grid of frame_grid.h in GetFeaturesInArea's order (src/Frame.cc:645-714).  The other matchers have files of
// their own: bf2nn_, search_init_, bow_, frame_ and tri_kernels.hip.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "frame_grid.h"
#include "match_common.h"
#include <climits>
#include <cstdlib>

// ---------------------------------------------------------------------------- SearchByProjection
// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), ORBmatcher.cc:1965-2181, Nleft == -1.
// One wave per frame pair.  The Frame grid (Frame.cc:377-408) is built in LDS as a CSR: cells are numbered
// ix*48+iy, so the cells (ix, r0..r1) that GetFeaturesInArea visits for one column are one contiguous run of
// the item list, and concatenating the runs of columns c0..c1 IS the function's visiting order (Frame.cc:
// 676-711).  Per query the lanes own one grid column each, a wave scan places the runs, and the candidates
// are then evaluated one per lane with key = distance << 12 | position ("first candidate wins", :2051-2055).
// The query loop is sequential: a keypoint claimed by a map point with observations drops out of later
// queries (:2037-2039).
#define SBP_CAP 2048          // keypoints / queries per frame of the replay form (its keys carry 11-bit positions and indices)
#define SBP_SEQ_CAP 8192      // ... of the sequential kernel, LDS permitting (17 B per keypoint + 3 B per query + the grid: see sbp_launch)
#define SBP_CAND_CAP 4096     // candidates of one query (12-bit position in its key)
// Register-resident sequential loop of SearchByProjection (both modes, frames of one camera, at most 64 * NS keypoints inside the
// grid).  The CSR grid orders the train keypoints by (grid column, row, rank) = GetFeaturesInArea's visit order; slot s of lane l
// holds the keypoint at CSR position 64 s + l -- position, cell, octave, holder state, uRight and descriptor in VGPRs.  A slot
// covers a contiguous range of grid columns, so a query only evaluates the 2..4 slots its window's columns intersect (uniform
// test), branch-free on all 64 lanes: cell-range + level + distance + holder + uRight gates, Hamming distance, key =
// distance << 12 | CSR position (the old candidate list's order).  No candidate list, no LDS or global access and no barrier
// in the chain (cycle counters, -DSBP_PROF: the list was 49 % of a query's 5200 cycles, the evaluation with its descriptor
// fetches 30 %).  Returns nmatches; writes qm[] and the final holder[] to LDS for the rotation check that follows.
template <int NS, bool UR>
__device__ __forceinline__ int sbp_register_loop(int lane, int n_items, int nq, const orbhip_proj_query *Q, const uint4 *dQ, const uint4 *dT,
                                                 const float *uright, const float *kx, const float *ky, const uint8_t *oct, const uint16_t *items,
                                                 const uint16_t *cell_of, int16_t *holder, int16_t *qm,
                                                 float min_x, float min_y, float inv_w, float inv_h, int th_high, int mode, float nn_ratio)
{
    float fkx[NS], fky[NS], fur[UR ? NS : 1]; uint32_t fpk[NS]; int fh[NS], fi[NS]; uint4 fd0[NS], fd1[NS];
    int slo[NS], shi[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int p = 64 * s + lane;
        const bool v = p < n_items;
        const int i2 = v ? (int)items[p] : 0;                                                          // (row 0 of the pair's arrays exists also for an empty frame)
        fi[s] = i2; fkx[s] = kx[i2]; fky[s] = ky[i2];
        const int cell = cell_of[i2], cx = (int)(((uint32_t)cell * 43691u) >> 21), cy = cell - SI_ROWS * cx;     // cell / 48, exact for cell < 3072
        fpk[s] = v ? (uint32_t)cx | ((uint32_t)cy << 7) | ((uint32_t)oct[i2] << 13) : 127u;          // column 127: in no window
        fh[s] = holder[i2]; if (UR) fur[s] = uright[i2];
        fd0[s] = dT[2 * i2]; fd1[s] = dT[2 * i2 + 1];
        const int lastl = min(63, n_items - 1 - 64 * s);                                              // uniform; < 0: empty slot
        slo[s] = lastl >= 0 ? __builtin_amdgcn_readlane(cx, 0) : 127;
        shi[s] = lastl >= 0 ? __builtin_amdgcn_readlane(cx, lastl) : -1;
    }
    int nmatches = 0;
    // the query records and descriptors are fetched two queries ahead
    orbhip_proj_query q1 = Q[0], q2 = Q[min(1, nq - 1)];
    uint4 a1_0 = dQ[0], a1_1 = dQ[1], a2_0 = dQ[2 * min(1, nq - 1)], a2_1 = dQ[2 * min(1, nq - 1) + 1];
    for (int t = 0; t < nq; t++) {
        const orbhip_proj_query qq = q1;
        const uint4 a0 = a1_0, a1 = a1_1;
        q1 = q2; a1_0 = a2_0; a1_1 = a2_1;
        { const int tn = min(t + 2, nq - 1); q2 = Q[tn]; a2_0 = dQ[2 * tn]; a2_1 = dQ[2 * tn + 1]; }
        const float x = qq.u, y = qq.v, r = qq.radius;
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        if (c0 >= SI_COLS) continue;
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        if (c1 < 0) continue;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        if (r0 >= SI_ROWS) continue;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        if (r1 < 0) continue;
        c0 = __builtin_amdgcn_readfirstlane(c0); c1 = __builtin_amdgcn_readfirstlane(c1);
        const bool check_lv = qq.min_level > 0 || qq.max_level >= 0;            // Frame.cc:676
        const uint32_t cw = (uint32_t)(c1 - c0), rh = (uint32_t)(r1 - r0);
        uint32_t lk1 = 0xFFFFFFFFu, lk2 = 0xFFFFFFFFu, pay1 = 0, pay2 = 0; int sl1 = 0;    // per lane: two smallest keys, their (index | octave << 16), the best's slot
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (shi[s] < c0 || slo[s] > c1) continue;                           // uniform: no keypoint of this slot in the window's columns
            const uint32_t dcx = (fpk[s] & 127u) - (uint32_t)c0, dcy = ((fpk[s] >> 7) & 63u) - (uint32_t)r0;
            const int o = (int)(fpk[s] >> 13), h = fh[s];
            // (bitwise &: no short-circuit branches -- every gate is a compare, the combination scalar logic)
            bool ok = (dcx <= cw) & (dcy <= rh);
            ok = ok & !((int)check_lv & ((int)(o < qq.min_level) | ((int)(qq.max_level >= 0) & (int)(o > qq.max_level))));   // Frame.cc:693-701
            ok = ok & (bool)((int)(fabsf(__fsub_rn(fkx[s], x)) < r) & (int)(fabsf(__fsub_rn(fky[s], y)) < r));   // Frame.cc:704-708
            ok = ok & !((h <= -2) | ((h >= 0) & ((h & 1) != 0)));                                       // ORBmatcher.cc:2037-2039 / 96-98
            if (UR) ok = ok & !((fur[s] > 0) & (fabsf(__fsub_rn(qq.ur, fur[s])) > r));                  // ORBmatcher.cc:2041-2047 / 100-105
            const int dist = hamming256(a0, a1, fd0[s], fd1[s]);
            const uint32_t key = ok ? ((uint32_t)dist << 12) | (uint32_t)(64 * s + lane) : 0xFFFFFFFFu;
            const uint32_t pay = (uint32_t)fi[s] | ((uint32_t)o << 16);
            const bool b1 = key < lk1, b2 = key < lk2;
            pay2 = b1 ? pay1 : (b2 ? pay : pay2); lk2 = b1 ? lk1 : (b2 ? key : lk2);
            pay1 = b1 ? pay : pay1; sl1 = b1 ? s : sl1; lk1 = b1 ? key : lk1;
        }
        const uint32_t key = wave_min_u32_dpp(lk1);
        if (key == 0xFFFFFFFFu) continue;
        bool accept = (int)(key >> 12) <= th_high && (int)(key >> 12) < 256;                         // ORBmatcher.cc:2030,2058 / 85,131
        const unsigned long long own1 = __ballot(lk1 == key);
        const int ol = __builtin_amdgcn_readfirstlane(__ffsll((long long)own1) - 1);
        const int bsl = __builtin_amdgcn_readlane(sl1, ol);
        if (accept && mode == 1) {
            // local-map variant (ORBmatcher.cc:131-137): ratio test against the second best when it is of the same octave; the second
            // smallest key is the minimum over the winner's runner-up and every other lane's best (keys are unique)
            const uint32_t c2 = lk1 == key ? lk2 : lk1, cp2 = lk1 == key ? pay2 : pay1;
            const uint32_t key2 = wave_min_u32_dpp(c2);
            const int best_lv = (int)((uint32_t)__builtin_amdgcn_readlane((int)pay1, ol) >> 16);
            int lv2 = -1, d2 = 256;
            if (key2 != 0xFFFFFFFFu && (int)(key2 >> 12) < 256) {
                d2 = (int)(key2 >> 12);
                const unsigned long long own2 = __ballot(c2 == key2);
                const int ol2 = __builtin_amdgcn_readfirstlane(__ffsll((long long)own2) - 1);
                lv2 = (int)((uint32_t)__builtin_amdgcn_readlane((int)cp2, ol2) >> 16);
            }
            if (best_lv == lv2 && (float)(int)(key >> 12) > __fmul_rn(nn_ratio, (float)d2)) accept = false;
        }
        if (accept) {
            const int best = (int)((uint32_t)__builtin_amdgcn_readlane((int)pay1, ol) & 0xFFFFu);
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (bsl == s) { if (lane == ol) fh[s] = (t << 1) | (qq.has_obs & 1); }          // uniform slot test
            if (lane == 0) qm[t] = (int16_t)best;
            nmatches++;
        }
    }
    // the holder states go back to LDS for the rotation check and the final write-out
#pragma unroll
    for (int s = 0; s < NS; s++) if (64 * s + lane < n_items) holder[fi[s]] = (int16_t)fh[s];
    return nmatches;
}

#ifdef SBP_PROF
__device__ long long g_sbp_prof[8];           // debug build only (EXTRA=-DSBP_PROF): cycles of setup / candidate list / evaluation / update / tail of pair 0; queries, candidates
#define SBP_T(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const long long t_ = clock64(); g_sbp_prof[i] += t_ - t_prev; t_prev = t_; } } while (0)
extern "C" int orbhip_debug_sbp_prof(long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_sbp_prof), 64) != hipSuccess) return ORBHIP_E_HIP;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sbp_prof), z, 64) != hipSuccess) return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
#else
#define SBP_T(i) do { } while (0)
#endif
template <bool DESC_LDS>
__global__ __launch_bounds__(64) void k_search_by_projection(const orbhip_proj_query *q_, const uint8_t *descq_, const int32_t *nq_, int max_q,
                                                             const orbhip_keypoint *kp_, const uint8_t *desc_, const float *uright_,
                                                             const int32_t *n_, int max_n, size_t kp_stride,
                                                             float min_x, float min_y, float max_x, float max_y,
                                                             int th_high, int check_ori, int mode, float nn_ratio, int cap_n, int cap_q,
                                                             int32_t *tm_, int32_t *nmatches_, int32_t *status,
                                                             const int32_t *nleft_, const int32_t *mirror_, int ncells, const int32_t *redo_)
{
    // dynamic LDS carved by the launcher's capacities (cap_n keypoints, cap_q queries per pair): small frames keep
    // four pairs per CU resident
    extern __shared__ __attribute__((aligned(16))) uint8_t sbp_lds[];
    uint32_t *cell_start = reinterpret_cast<uint32_t *>(sbp_lds);                   // [ncells + 1]: SBP_CELLS, twice that for rig frames
    float *kx = reinterpret_cast<float *>(cell_start + ncells + 1), *ky = kx + cap_n;
    int16_t *holder = reinterpret_cast<int16_t *>(ky + cap_n);                       // -1 free, -2 pre-held, else (query << 1 | has_obs)
    // (the candidate list of ONE query never needs more than 4096 entries -- its position travels in 12 bits of the key -- so keyframes of
    // up to ~7 600 keypoints fit: the 5 x nFeatures keypoints of a monocular map's first two keyframes, Tracking.cc:210)
    const int cap_c = cap_n < SBP_CAND_CAP ? cap_n : SBP_CAND_CAP;
    uint16_t *items = reinterpret_cast<uint16_t *>(holder + cap_n), *cand = items + cap_n, *cell_of = cand + cap_c, *rank_of = cell_of + cap_n;
    int16_t *qm = reinterpret_cast<int16_t *>(rank_of + cap_n);                      // query -> claimed keypoint
    int8_t *qbin = reinterpret_cast<int8_t *>(qm + cap_q);
    uint8_t *oct = reinterpret_cast<uint8_t *>(qbin + cap_q);
    // optional: the train descriptors too (32 B each) -- removes the one global round trip left in every query; used when
    // the launch is small enough that fewer resident pairs per CU do not matter
    uint4 *dlds = reinterpret_cast<uint4 *>(sbp_lds + ((sizeof(uint32_t) * ((size_t)ncells + 1) + (size_t)cap_n * 17 + (size_t)cap_c * 2 + (size_t)cap_q * 3 + 15) & ~(size_t)15));
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (redo_ && !redo_[pair]) return;                       // the low-latency form (k_sbp_replay) has done this pair
#ifdef SBP_PROF
    long long t_prev = clock64();
#endif
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const int n = n_[pair], nq = nq_[pair];
    // rig frames (Nleft != -1): keypoints [0, nleft) are the left camera's, [nleft, n) the right camera's; a query carries the camera
    // it searches in bit 1 of has_obs; mirror[i] = the same point's keypoint in the other camera (mvLeftToRightMatch / mvRightToLeftMatch
    // as frame-wide indices) or -1
    const int nleft = nleft_ ? nleft_[pair] : -1;
    const int32_t *mirror = mirror_ ? mirror_ + (size_t)pair * max_n : nullptr;
    const orbhip_proj_query *Q = q_ + (size_t)pair * max_q;
    const uint4 *dQ = reinterpret_cast<const uint4 *>(descq_ + (size_t)pair * max_q * 32);
    const orbhip_keypoint *kp = kp_ + (size_t)pair * kp_stride;
    const uint4 *dT = reinterpret_cast<const uint4 *>(desc_ + (size_t)pair * kp_stride * 32);
    const float *uright = uright_ ? uright_ + (size_t)pair * kp_stride : nullptr;
    int32_t *tm = tm_ + (size_t)pair * max_n;
    if (n > cap_n || nq > cap_q || n > max_n || nq > max_q) {
        if (lane == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; }
        return;
    }
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x));       // Frame.cc:334-335
    const float inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    for (int c = lane; c <= ncells; c += 64) cell_start[c] = 0;
    for (int t = lane; t < nq; t += 64) { qm[t] = -1; qbin[t] = -1; }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        holder[i] = tm[i] == -1 ? (int16_t)-1 : (int16_t)-2;
        if (DESC_LDS) { dlds[2 * i] = dT[2 * i]; dlds[2 * i + 1] = dT[2 * i + 1]; }
    }
    sbp_build_grid(cell_start, kx, ky, oct, items, cell_of, rank_of, kp, n, min_x, min_y, inv_w, inv_h, lane, ncells, nleft);
    SBP_T(0);
    // ---- sequential query loop (ORBmatcher.cc:1987-2088)
    int nmatches = 0;
    const int n_items = (int)cell_start[ncells];
    if (nleft < 0 && !mirror && n_items <= 16 * 64 && nq > 0) {
        nmatches = uright ? sbp_register_loop<16, true>(lane, n_items, nq, Q, dQ, dT, uright, kx, ky, oct, items, cell_of, holder, qm, min_x, min_y, inv_w, inv_h,
                                                        th_high, mode, nn_ratio)
                          : sbp_register_loop<16, false>(lane, n_items, nq, Q, dQ, dT, uright, kx, ky, oct, items, cell_of, holder, qm, min_x, min_y, inv_w, inv_h,
                                                         th_high, mode, nn_ratio);
    } else {
    // the next query's record and descriptor are fetched one iteration ahead (their latency overlaps this query's work)
    orbhip_proj_query qn = Q[0];
    uint4 n0 = dQ[0], n1 = dQ[1];
    for (int t = 0; t < nq; t++) {
        const orbhip_proj_query qq = qn;
        const uint4 a0 = n0, a1 = n1;
        if (t + 1 < nq) { qn = Q[t + 1]; n0 = dQ[2 * t + 2]; n1 = dQ[2 * t + 3]; }
        const float x = qq.u, y = qq.v, r = qq.radius;
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        if (c0 >= SI_COLS) continue;
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        if (c1 < 0) continue;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        if (r0 >= SI_ROWS) continue;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        if (r1 < 0) continue;
        // lane = grid column c0+lane: its cells r0..r1 are one run of `items` (rig: the queried camera's half of the cells)
        const int cbase = (nleft >= 0 && (qq.has_obs & 2)) ? SBP_CELLS : 0;
        int start = 0, len = 0;
        if (c0 + lane <= c1) {
            start = (int)cell_start[cbase + (c0 + lane) * SI_ROWS + r0];
            len = (int)cell_start[cbase + (c0 + lane) * SI_ROWS + r1 + 1] - start;
        }
        const int inc = wave_scan_add_dpp(len);                      // DPP scans / reductions: no LDS round trips in the per-query chain
        const int off = inc - len, total = __builtin_amdgcn_readlane(inc, 63);
        if (total == 0) continue;
        if (total > cap_c) { if (lane == 0) atomicExch(status, ORBHIP_E_CAPACITY); continue; }      // > 4096 keypoints in one search window
        const int maxlen = wave_max_dpp(len);
        for (int j = 0; j < maxlen; j++) if (j < len) cand[off + j] = items[start + j];
        __syncthreads();
        SBP_T(1);
        const bool check_lv = qq.min_level > 0 || qq.max_level >= 0;            // Frame.cc:676
        uint32_t key = 0xFFFFFFFFu, key2 = 0xFFFFFFFFu;                         // the two smallest (distance << 12 | position)
        for (int k0 = 0; k0 < total; k0 += 64) {
            const int k = k0 + lane;
            if (k < total) {
                const int i2 = cand[k];
                // the descriptor is fetched together with the keypoint's other data (one latency instead of two on the chain)
                const uint4 t0 = DESC_LDS ? dlds[2 * i2] : dT[2 * i2], t1 = DESC_LDS ? dlds[2 * i2 + 1] : dT[2 * i2 + 1];
                const int o = oct[i2], h = holder[i2];
                bool ok = !(check_lv && (o < qq.min_level || (qq.max_level >= 0 && o > qq.max_level)));   // Frame.cc:693-701
                ok = ok && fabsf(__fsub_rn(kx[i2], x)) < r && fabsf(__fsub_rn(ky[i2], y)) < r;           // Frame.cc:704-708
                ok = ok && !(h <= -2 || (h >= 0 && (h & 1)));                                              // ORBmatcher.cc:2037-2039 / 96-98
                if (ok && uright) {
                    const float ur2 = uright[i2];
                    if (ur2 > 0 && fabsf(__fsub_rn(qq.ur, ur2)) > r) ok = false;                           // ORBmatcher.cc:2041-2047 / 100-105
                }
                if (ok) {
                    const int dist = hamming256(a0, a1, t0, t1);
                    const uint32_t kk = ((uint32_t)dist << 12) | (uint32_t)k;
                    key2 = min(key2, max(key, kk));
                    key = min(key, kk);
                }
            }
        }
        wave_min2_u32_dpp(key, key2);
        SBP_T(2);
#ifdef SBP_PROF
        if (blockIdx.x == 0 && threadIdx.x == 0) { g_sbp_prof[5] += 1; g_sbp_prof[6] += total; }
#endif
        bool accept = key != 0xFFFFFFFFu && (int)(key >> 12) <= th_high && (int)(key >> 12) < 256;       // ORBmatcher.cc:2030,2058 / 85,131
        if (accept && mode == 1) {
            // local-map variant (ORBmatcher.cc:131-137): ratio test against the second best of the same octave.
            // "second best" of the reference's scan == second smallest key (strict <, first candidate wins ties)
            const int best_lv = oct[cand[key & 0xFFFu]];
            int d2 = 256, lv2 = -1;
            if (key2 != 0xFFFFFFFFu && (int)(key2 >> 12) < 256) { d2 = (int)(key2 >> 12); lv2 = oct[cand[key2 & 0xFFFu]]; }
            if (best_lv == lv2 && (float)(int)(key >> 12) > __fmul_rn(nn_ratio, (float)d2)) accept = false;
        }
        if (accept) {
            if (lane == 0) {
                const int best = cand[key & 0xFFFu];
                holder[best] = (int16_t)((t << 1) | (qq.has_obs & 1));
                qm[t] = (int16_t)best;
            }
            nmatches++;
            if (mirror) {                                                       // also the stereo observation in the other camera (:142-146, :203-207)
                const int m = mirror[cand[key & 0xFFFu]];
                if (m >= 0) { if (lane == 0) holder[m] = (int16_t)((t << 1) | (qq.has_obs & 1)); nmatches++; }
            }
        }
        __syncthreads();                                                        // cand / holder reused by the next query
        SBP_T(3);
    }
    }
    __syncthreads();
    // ---- rotation consistency (ORBmatcher.cc:2156-2178): every histogram entry of a dropped bin clears its
    // keypoint (also when a later query re-claimed it) and counts once.  Bins (ORBmatcher.cc:2064-2084) are computed
    // here in parallel for all matches instead of inside the sequential loop (one dependent global read less per query).
    if (check_ori) {
        for (int t = lane; t < nq; t += 64) {
            const int best = qm[t];
            if (best < 0) continue;
            const int bin = rot_bin(Q[t].angle, kp[best].angle);
            atomicAdd(&hist[bin], 1); qbin[t] = (int8_t)bin;
        }
        __syncthreads();
        if (lane == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        int removed = 0;
        for (int t = lane; t < nq; t += 64) {
            const int b = qbin[t];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            holder[qm[t]] = -1; removed++;
        }
        removed = wave_sum_dpp(removed);
        nmatches -= removed;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) { const int h = holder[i]; tm[i] = h >= 0 ? (h >> 1) : h; }
    if (lane == 0) nmatches_[pair] = nmatches;
    SBP_T(4);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Low-latency form of SearchByProjection (both modes, single-camera frames) for calls with FEW frame pairs -- Tracking calls the
// matcher with one.  The register / LDS loops above walk the queries one after the other on ONE wave per pair (~1.2 us per query: 1.2 ms
// for a frame, whatever the batch); here the expensive part of a query -- window, gates, Hamming distances -- does not depend on the
// claim rule and is evaluated for ALL queries at once, over the whole chip:
//   k_sbp_prep        one wave per pair: the Frame grid as a CSR (sbp_build_grid), written out in CSR order: per position a record
//                     {x, y, cell | octave | pre-held, uRight}, the keypoint index, the descriptor, and the first position of every grid column;
//   k_sbp_candidates  one wave per query: the window's columns are ONE contiguous range of CSR positions; every position in it is gated
//                     (cell range, level, |dx|,|dy| < r, pre-held, uRight) and its Hamming distance taken; the keys
//                     distance << 22 | position << 11 | keypoint index are sorted (rank by counting, in LDS) and the SBPL_K smallest stored;
//   k_sbp_replay      one wave per pair replays the claim rule (ORBmatcher.cc:2037-2039 / :96-98) over the sorted lists, 64 queries per
//                     trip, one per lane: a lane's best (and, local-map mode, second best) is its first (two) list entries whose keypoint no
//                     EARLIER query with observations holds -- claims only ever block more keypoints, so a lane's cursor only moves forward.
//                     Inside a trip the lanes are speculative: every lane publishes its claim (LDS atomicMin of the lane id per keypoint), the
//                     prefix of lanes up to the first one whose best / second best was claimed by an earlier lane is final, the others look
//                     again.  A trip needs 1 + (number of conflicts) rounds of a few LDS operations.
// The result is the sequential loop's, bit for bit (same candidate sets, same key order, same claim rule); a query whose list was cut at
// SBPL_K entries and runs out of them makes its pair fall back to the sequential kernel (flag per pair, read on the device).
#define SBPL_K 32                  // list entries kept per query
#define SBPL_BUF 512               // candidates a query may have before the pair falls back
struct SbpWork {
    float4 *rec;                   // [pairs][cap_n]   CSR order: x, y, bits(cx | cy << 7 | octave << 13 | pre-held << 17), uRight
    uint4 *desc;                   // [pairs][cap_n][2]
    uint16_t *idx;                 // [pairs][cap_n]   keypoint index at a CSR position
    int32_t *col_start;            // [pairs][SI_COLS + 1]
    uint32_t *lists;               // [pairs][chunks][SBPL_K][64]   (transposed: lane = query inside a trip of 64)
    int32_t *count;                // [pairs][cap_q]   candidates of the query (may exceed SBPL_K; INT_MAX: more than SBPL_BUF)
    int32_t *redo;                 // [pairs]          1 = the sequential kernel must process this pair
    int cap_n, cap_q, chunks;
};

__global__ __launch_bounds__(64) void k_sbp_prep(const orbhip_keypoint *kp_, const uint8_t *desc_, const float *uright_, const int32_t *n_, int max_n,
                                                 size_t kp_stride, float min_x, float min_y, float max_x, float max_y, const int32_t *tm_, SbpWork W,
                                                 int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sbp_lds[];
    uint32_t *cell_start = reinterpret_cast<uint32_t *>(sbp_lds);
    float *kx = reinterpret_cast<float *>(cell_start + SBP_CELLS + 1), *ky = kx + W.cap_n;
    uint16_t *items = reinterpret_cast<uint16_t *>(ky + W.cap_n), *cell_of = items + W.cap_n, *rank_of = cell_of + W.cap_n;
    uint8_t *oct = reinterpret_cast<uint8_t *>(rank_of + W.cap_n);
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int n = n_[pair];
    int32_t *cs = W.col_start + (size_t)pair * (SI_COLS + 1);
    if (n > W.cap_n || n > max_n) {
        if (lane == 0) { atomicExch(status, ORBHIP_E_CAPACITY); W.redo[pair] = 1; }
        for (int c = lane; c <= SI_COLS; c += 64) cs[c] = 0;
        return;
    }
    const orbhip_keypoint *kp = kp_ + (size_t)pair * kp_stride;
    const uint4 *dT = reinterpret_cast<const uint4 *>(desc_ + (size_t)pair * kp_stride * 32);
    const float *uright = uright_ ? uright_ + (size_t)pair * kp_stride : nullptr;
    const int32_t *tm = tm_ + (size_t)pair * max_n;
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x)), inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    for (int c = lane; c <= SBP_CELLS; c += 64) cell_start[c] = 0;
    __syncthreads();
    sbp_build_grid(cell_start, kx, ky, oct, items, cell_of, rank_of, kp, n, min_x, min_y, inv_w, inv_h, lane);
    const int n_items = (int)cell_start[SBP_CELLS];
    float4 *rec = W.rec + (size_t)pair * W.cap_n;
    uint4 *dC = W.desc + (size_t)pair * W.cap_n * 2;
    uint16_t *idx = W.idx + (size_t)pair * W.cap_n;
    for (int p = lane; p < n_items; p += 64) {
        const int i = items[p];
        const int cell = cell_of[i], cx = (int)(((uint32_t)cell * 43691u) >> 21), cy = cell - SI_ROWS * cx;
        const uint32_t bits = (uint32_t)cx | ((uint32_t)cy << 7) | ((uint32_t)oct[i] << 13) | ((tm[i] != -1) ? (1u << 17) : 0u);
        rec[p] = make_float4(kx[i], ky[i], __uint_as_float(bits), uright ? uright[i] : -1.0f);
        idx[p] = (uint16_t)i;
        dC[2 * p] = dT[2 * i]; dC[2 * p + 1] = dT[2 * i + 1];
    }
    for (int c = lane; c <= SI_COLS; c += 64) cs[c] = (int32_t)cell_start[c * SI_ROWS];
    if (lane == 0) W.redo[pair] = 0;
}

__global__ __launch_bounds__(256) void k_sbp_candidates(const orbhip_proj_query *q_, const uint8_t *descq_, const int32_t *nq_, int max_q,
                                                        float min_x, float min_y, float max_x, float max_y, int use_ur, SbpWork W)
{
    __shared__ uint32_t kbuf_all[4][SBPL_BUF];
    const int pair = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + w;
    const int nq = nq_[pair];
    if (t >= nq || nq > W.cap_q || nq > max_q) return;
    uint32_t *kbuf = kbuf_all[w];
    const orbhip_proj_query qq = q_[(size_t)pair * max_q + t];
    const uint4 *dQ = reinterpret_cast<const uint4 *>(descq_ + ((size_t)pair * max_q + t) * 32);
    const uint4 a0 = dQ[0], a1 = dQ[1];
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x)), inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    const float x = qq.u, y = qq.v, r = qq.radius;
    int32_t *count = W.count + (size_t)pair * W.cap_q;
    int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;                   // Frame.cc:656-674
    int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
    int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
    int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
    if (c0 >= SI_COLS || c1 < 0 || r0 >= SI_ROWS || r1 < 0) { if (lane == 0) count[t] = 0; return; }
    const int32_t *cs = W.col_start + (size_t)pair * (SI_COLS + 1);
    const int p0 = cs[c0], p1 = cs[c1 + 1];
    const float4 *rec = W.rec + (size_t)pair * W.cap_n;
    const uint4 *dC = W.desc + (size_t)pair * W.cap_n * 2;
    const uint16_t *idx = W.idx + (size_t)pair * W.cap_n;
    const bool check_lv = qq.min_level > 0 || qq.max_level >= 0;                                                     // Frame.cc:676
    const uint32_t cw = (uint32_t)(c1 - c0), rh = (uint32_t)(r1 - r0);
    int total = 0;
    for (int pb = p0; pb < p1; pb += 64) {
        const int p = pb + lane;
        bool ok = p < p1;
        uint32_t key = 0xFFFFFFFFu;
        if (ok) {
            const float4 k = rec[p];
            const uint32_t bits = __float_as_uint(k.z);
            const uint32_t dcx = (bits & 127u) - (uint32_t)c0, dcy = ((bits >> 7) & 63u) - (uint32_t)r0;
            const int o = (int)((bits >> 13) & 15u);
            ok = (dcx <= cw) & (dcy <= rh);
            ok = ok & !((int)check_lv & ((int)(o < qq.min_level) | ((int)(qq.max_level >= 0) & (int)(o > qq.max_level))));   // Frame.cc:693-701
            ok = ok & (bool)((int)(fabsf(__fsub_rn(k.x, x)) < r) & (int)(fabsf(__fsub_rn(k.y, y)) < r));                    // Frame.cc:704-708
            ok = ok & !((bits >> 17) & 1u);                                                                                  // holds a map point already (:2037 / :96 on entry)
            if (use_ur) ok = ok & !((k.w > 0) & (fabsf(__fsub_rn(qq.ur, k.w)) > r));                                        // ORBmatcher.cc:2041-2047 / 100-105
            if (ok) {
                const int dist = hamming256(a0, a1, dC[2 * p], dC[2 * p + 1]);
                key = ((uint32_t)dist << 22) | ((uint32_t)p << 11) | (uint32_t)idx[p];
            }
        }
        const unsigned long long m = __ballot(ok);
        const int before = __popcll(m & ((1ull << lane) - 1));
        if (ok && total + before < SBPL_BUF) kbuf[total + before] = key;
        total += __popcll(m);
    }
    if (total > SBPL_BUF) { if (lane == 0) count[t] = 0x7FFFFFFF; return; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // rank by counting (keys are unique): the SBPL_K smallest go to the list in order
    uint32_t *L = W.lists + (((size_t)pair * W.chunks + (t >> 6)) * SBPL_K) * 64 + (t & 63);
    for (int e = lane; e < total; e += 64) {
        const uint32_t mine = kbuf[e];
        int rank = 0;
        for (int j = 0; j < total; j++) rank += kbuf[j] < mine;
        if (rank < SBPL_K) L[(size_t)rank * 64] = mine;
    }
    if (lane == 0) count[t] = total;
}

__global__ __launch_bounds__(64) void k_sbp_replay(const orbhip_proj_query *q_, const int32_t *nq_, int max_q, const orbhip_keypoint *kp_,
                                                   const int32_t *n_, int max_n, size_t kp_stride, int th_high, int check_ori, int mode, float nn_ratio,
                                                   SbpWork W, int32_t *tm_, int32_t *nmatches_)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sbp_lds[];
    int32_t *holder = reinterpret_cast<int32_t *>(sbp_lds);                         // [cap_n]  -1 free, -2 pre-held, else query << 1 | has_obs
    int32_t *owner = holder + W.cap_n;                                               // [cap_n]  lowest lane of this round that claims the keypoint (64: none)
    int16_t *qm = reinterpret_cast<int16_t *>(owner + W.cap_n);                      // [cap_q]
    uint8_t *oct = reinterpret_cast<uint8_t *>(qm + W.cap_q);                        // [cap_n]
    int8_t *qbin = reinterpret_cast<int8_t *>(oct + W.cap_n);                        // [cap_q]
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (W.redo[pair]) return;                                                        // (capacity: the sequential kernel reports it)
    const int n = n_[pair], nq = nq_[pair];
    if (nq > W.cap_q || nq > max_q) { if (lane == 0) W.redo[pair] = 1; return; }
    const orbhip_proj_query *Q = q_ + (size_t)pair * max_q;
    const orbhip_keypoint *kp = kp_ + (size_t)pair * kp_stride;
    int32_t *tm = tm_ + (size_t)pair * max_n;
    const int32_t *count = W.count + (size_t)pair * W.cap_q;
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    for (int i = lane; i < n; i += 64) { holder[i] = tm[i] == -1 ? -1 : -2; owner[i] = 64; oct[i] = (uint8_t)kp[i].octave; }
    for (int t = lane; t < nq; t += 64) { qm[t] = -1; qbin[t] = -1; }
    __syncthreads();
    int nmatches = 0;
    bool give_up = false;
    for (int t0 = 0; t0 < nq && !give_up; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < nq;
        const uint32_t *L = W.lists + (((size_t)pair * W.chunks + (t0 >> 6)) * SBPL_K) * 64 + lane;
        const int cnt_all = valid ? count[t] : 0;
        const int cnt = min(cnt_all, SBPL_K);
        const int ho = valid ? (Q[t].has_obs & 1) : 0;
        uint32_t kr0 = 0xFFFFFFFFu, kr1 = 0xFFFFFFFFu, kr2 = 0xFFFFFFFFu, kr3 = 0xFFFFFFFFu;      // the head of the list in registers (one batch of loads)
        if (cnt > 0) kr0 = L[0];
        if (cnt > 1) kr1 = L[64];
        if (cnt > 2) kr2 = L[128];
        if (cnt > 3) kr3 = L[192];
        if (__ballot(cnt_all == 0x7FFFFFFF)) { give_up = true; break; }
        int ptr = 0;
        bool fin = !valid || cnt == 0;
#define SBPL_ENTRY(p) ((p) == 0 ? kr0 : (p) == 1 ? kr1 : (p) == 2 ? kr2 : (p) == 3 ? kr3 : L[(size_t)(p) * 64])
#define SBPL_BLOCKED(key) (holder[(key) & 0x7FFu] >= 0 && (holder[(key) & 0x7FFu] & 1))
        while (true) {
            uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
            bool accept = false, starved = false;
            if (!fin) {
                while (ptr < cnt) { const uint32_t k = SBPL_ENTRY(ptr); if (!SBPL_BLOCKED(k)) { k1 = k; break; } ptr++; }
                if (k1 == 0xFFFFFFFFu) starved = cnt_all > SBPL_K;                    // ran out of a truncated list
                else {
                    const int d1 = (int)(k1 >> 22);
                    accept = d1 <= th_high && d1 < 256;                                // ORBmatcher.cc:2058 / :131
                    if (accept && mode == 1) {                                         // ratio test against the second best of the same octave (:131-137)
                        int p2 = ptr + 1;
                        while (p2 < cnt) { const uint32_t k = SBPL_ENTRY(p2); if (!SBPL_BLOCKED(k)) { k2 = k; break; } p2++; }
                        if (k2 == 0xFFFFFFFFu) starved = cnt_all > SBPL_K;
                        else {
                            const int d2 = (int)(k2 >> 22);
                            // (a candidate at distance 256 is no second best: `dist < bestDist2` with bestDist2 = 256, :119 -- as in the sequential loops)
                            if (d2 < 256 && oct[k1 & 0x7FFu] == oct[k2 & 0x7FFu] && (float)d1 > __fmul_rn(nn_ratio, (float)d2)) accept = false;
                        }
                    }
                }
            }
            if (__ballot(starved)) { give_up = true; break; }
            // speculative claims of this round: the lowest lane that wants a keypoint (only claims of points WITH observations block others)
            const bool claims = !fin && accept && ho;
            if (claims) atomicMin(&owner[k1 & 0x7FFu], lane);
            __syncthreads();
            bool conflict = false;
            if (!fin) {
                if (k1 != 0xFFFFFFFFu) conflict = owner[k1 & 0x7FFu] < lane;
                if (k2 != 0xFFFFFFFFu) conflict = conflict || owner[k2 & 0x7FFu] < lane;
            }
            const unsigned long long cm = __ballot(conflict);
            const int f = cm ? __ffsll((long long)cm) - 1 : 64;                        // lanes below f are final
            __syncthreads();
            if (claims) owner[k1 & 0x7FFu] = 64;
            if (!fin && lane < f) {
                if (accept) {
                    // several final lanes may take one keypoint when the earlier ones carry no observations: the LAST query keeps it (:2061 / :140)
                    atomicMax(&holder[k1 & 0x7FFu], (t << 1) | ho);
                    qm[t] = (int16_t)(k1 & 0x7FFu);
                    nmatches++;
                }
                fin = true;
            }
            __syncthreads();
            if (f == 64) break;
        }
#undef SBPL_ENTRY
#undef SBPL_BLOCKED
    }
    if (give_up) { if (lane == 0) W.redo[pair] = 1; return; }                          // nothing written yet: the sequential kernel does this pair
    nmatches = wave_sum_dpp(nmatches);
    __syncthreads();
    if (check_ori) {                                                                   // rotation consistency, as in k_search_by_projection
        for (int t = lane; t < nq; t += 64) {
            const int best = qm[t];
            if (best < 0) continue;
            const int bin = rot_bin(Q[t].angle, kp[best].angle);
            atomicAdd(&hist[bin], 1); qbin[t] = (int8_t)bin;
        }
        __syncthreads();
        if (lane == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        int removed = 0;
        for (int t = lane; t < nq; t += 64) {
            const int b = qbin[t];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            holder[qm[t]] = -1; removed++;
        }
        nmatches -= wave_sum_dpp(removed);
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) { const int h = holder[i]; tm[i] = h >= 0 ? (h >> 1) : h; }
    if (lane == 0) nmatches_[pair] = nmatches;
}

// LDS of k_search_by_projection for the given row capacities (keypoints / queries per pair)
static size_t sbp_lds_bytes(int cap_n, int cap_q, int ncells)
{
    const int cap_c = cap_n < SBP_CAND_CAP ? cap_n : SBP_CAND_CAP;
    return sizeof(uint32_t) * ((size_t)ncells + 1) + (size_t)cap_n * (4 + 4 + 2 + 2 + 2 + 2 + 1) + (size_t)cap_c * 2 + (size_t)cap_q * (2 + 1) + 16;
}
static int sbp_launch(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q, const int32_t *d_nq, int max_q,
                      const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *d_u_right, const int32_t *d_n, int max_n,
                      size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x, float max_y, int th_high,
                      int check_orientation, int mode, float nn_ratio, int32_t *d_train_match, int32_t *d_nmatches,
                      const int32_t *d_nleft = nullptr, const int32_t *d_mirror = nullptr)
{
    // Frames / keyframes beyond the replay form's 2048 keypoints or queries (the two first keyframes of a monocular map carry 5 x nFeatures
    // keypoints, Tracking.cc:210; a loop's map points can be thousands of queries) take the sequential kernel alone, whose arrays are
    // sized by what LDS holds: 17 B per keypoint + 2 B per candidate slot + 3 B per query + the grid (round 4; round 3 refused > 2048)
    const bool big = max_n > SBP_CAP || max_q > SBP_CAP;
    const int lim = big ? SBP_SEQ_CAP : SBP_CAP;
    const int cap_n = ((max_n < lim ? max_n : lim) + 7) & ~7, cap_q = ((max_q < lim ? max_q : lim) + 7) & ~7;
    const int ncells = d_nleft ? 2 * SBP_CELLS : SBP_CELLS;
    const size_t base = sbp_lds_bytes(cap_n, cap_q, ncells), with_desc = base + (size_t)cap_n * 32;
    if (base > 160 * 1024 - 512) { orbhip_set_last_error_internal("SearchByProjection: frame too large for the LDS-resident grid (17 B per keypoint + 3 B per query <= ~145 KB)"); return ORBHIP_E_CAPACITY; }
    // descriptors in LDS when at most two rounds of workgroups are needed anyway (<= 2 pairs per CU resident is enough)
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    // The replay form first (candidate lists for all queries at once, then the claim rule replayed over them); a pair it cannot finish
    // (a truncated list ran dry, > SBPL_BUF candidates) is flagged and done by the sequential kernel below, which returns at once for the
    // others.  Measured (tools/sbp_sweep.py, ~1000 queries x ~1000 keypoints per pair): 1 pair 0.15 ms against 1.18 ms, 1023 pairs 0.69 ms
    // against 1.25 ms (last frame); 0.24 / 1.22 ms and 0.80 / 1.32 ms (local map).  Its work arena (lists + CSR copies, ~190 KB per pair
    // at 1000 keypoints) is capped at 1 GiB; beyond that, for rig frames, and when ORBHIP_SBP_PARALLEL_MAX_PAIRS says so, the sequential
    // kernel runs alone.
    const int par_max = getenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS") ? atoi(getenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS")) : (1 << 20);
    const size_t work_per_pair = (size_t)cap_n * (16 + 32 + 2) + 4 * (SI_COLS + 1) + 4 * (size_t)((cap_q + 63) / 64) * SBPL_K * 64 + 4 * (size_t)cap_q + 1024;
    const int32_t *d_redo = nullptr;
    orbhip_ctx_note_sbp_redo_internal(ctx, 0, 0);
    if (!big && !d_nleft && !d_mirror && pairs <= par_max && (size_t)pairs * work_per_pair <= ((size_t)1 << 30)) {
        SbpWork W;
        W.cap_n = cap_n; W.cap_q = cap_q; W.chunks = (cap_q + 63) / 64;
        const size_t o_rec = 0, o_desc = o_rec + align256(sizeof(float4) * (size_t)pairs * cap_n), o_idx = o_desc + align256(32 * (size_t)pairs * cap_n),
                     o_cs = o_idx + align256(2 * (size_t)pairs * cap_n), o_lists = o_cs + align256(4 * (size_t)pairs * (SI_COLS + 1)),
                     o_count = o_lists + align256(4 * (size_t)pairs * W.chunks * SBPL_K * 64), o_redo = o_count + align256(4 * (size_t)pairs * cap_q),
                     total = o_redo + align256(4 * (size_t)pairs);
        uint8_t *wb = (uint8_t *)orbhip_ctx_work_internal(ctx, total);
        if (!wb) return ORBHIP_E_HIP;
        W.rec = (float4 *)(wb + o_rec); W.desc = (uint4 *)(wb + o_desc); W.idx = (uint16_t *)(wb + o_idx); W.col_start = (int32_t *)(wb + o_cs);
        W.lists = (uint32_t *)(wb + o_lists); W.count = (int32_t *)(wb + o_count); W.redo = (int32_t *)(wb + o_redo);
        const size_t prep_lds = sizeof(uint32_t) * (SBP_CELLS + 1) + (size_t)cap_n * (4 + 4 + 2 + 2 + 2 + 1) + 16;
        const size_t rep_lds = (size_t)cap_n * (4 + 4 + 1) + (size_t)cap_q * (2 + 1) + 16;
        if (orb_lds_optin(reinterpret_cast<const void *>(k_sbp_prep), orbhip_ctx_device_internal(ctx), prep_lds) ||
            orb_lds_optin(reinterpret_cast<const void *>(k_sbp_replay), orbhip_ctx_device_internal(ctx), rep_lds)) return ORBHIP_E_HIP;
        hipLaunchKernelGGL(k_sbp_prep, dim3(pairs), dim3(64), prep_lds, st, d_kp, d_desc, d_u_right, d_n, max_n, frame_stride_kp, min_x, min_y, max_x, max_y,
                           d_train_match, W, orbhip_ctx_status_internal(ctx));
        hipLaunchKernelGGL(k_sbp_candidates, dim3((cap_q + 3) / 4, pairs), dim3(256), 0, st, d_q, d_desc_q, d_nq, max_q, min_x, min_y, max_x, max_y,
                           d_u_right ? 1 : 0, W);
        hipLaunchKernelGGL(k_sbp_replay, dim3(pairs), dim3(64), rep_lds, st, d_q, d_nq, max_q, d_kp, d_n, max_n, frame_stride_kp, th_high, check_orientation,
                           mode, nn_ratio, W, d_train_match, d_nmatches);
        d_redo = W.redo;
        orbhip_ctx_note_sbp_redo_internal(ctx, o_redo, pairs);
    }
    const bool desc_lds = with_desc <= 150 * 1024 && (size_t)pairs * with_desc <= (size_t)cus * 150 * 1024;
    const size_t lds = desc_lds ? with_desc : base;
    auto kern = desc_lds ? k_search_by_projection<true> : k_search_by_projection<false>;
    if (orb_lds_optin(reinterpret_cast<const void *>(kern), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(kern, dim3(pairs), dim3(64), lds, st, d_q, d_desc_q, d_nq,
                       max_q, d_kp, d_desc, d_u_right, d_n, max_n, frame_stride_kp, min_x, min_y, max_x, max_y, th_high,
                       check_orientation, mode, nn_ratio, cap_n, cap_q, d_train_match, d_nmatches, orbhip_ctx_status_internal(ctx), d_nleft, d_mirror, ncells,
                       d_redo);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

extern "C" int orbhip_search_by_projection_rig_device(orbhip_ctx *ctx, int mode, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                                      const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc,
                                                      const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n,
                                                      size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x, float max_y,
                                                      int th_high, float nn_ratio, int check_orientation, int32_t *d_train_match,
                                                      int32_t *d_nmatches)
{
    if (!ctx || (mode != 0 && mode != 1) || !d_q || !d_desc_q || !d_nq || !d_kp || !d_desc || !d_n || !d_nleft || pairs <= 0 || max_n <= 0 ||
        max_q <= 0 || !d_train_match || !d_nmatches || !(max_x > min_x) || !(max_y > min_y))
        return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    return sbp_launch(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, nullptr, d_n, max_n, frame_stride_kp, pairs, min_x, min_y, max_x, max_y,
                      th_high, mode == 0 ? check_orientation : 0, mode, nn_ratio, d_train_match, d_nmatches, d_nleft, mode == 1 ? d_mirror : nullptr);
}

extern "C" int orbhip_search_by_projection_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                                  const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp,
                                                  const uint8_t *d_desc, const float *d_u_right, const int32_t *d_n, int max_n,
                                                  size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x,
                                                  float max_y, int th_high, int check_orientation, int32_t *d_train_match,
                                                  int32_t *d_nmatches)
{
    if (!ctx || !d_q || !d_desc_q || !d_nq || !d_kp || !d_desc || !d_n || pairs <= 0 || max_n <= 0 || max_q <= 0 ||
        !d_train_match || !d_nmatches || !(max_x > min_x) || !(max_y > min_y))
        return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    return sbp_launch(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, frame_stride_kp, pairs, min_x, min_y,
                      max_x, max_y, th_high, check_orientation, 0, 0.0f, d_train_match, d_nmatches);
}

// ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, ...), ORBmatcher.cc:48-218 (Nleft == -1)
extern "C" int orbhip_search_local_map_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                              const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp,
                                              const uint8_t *d_desc, const float *d_u_right, const int32_t *d_n, int max_n,
                                              size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x,
                                              float max_y, int th_high, float nn_ratio, int32_t *d_train_match,
                                              int32_t *d_nmatches)
{
    if (!ctx || !d_q || !d_desc_q || !d_nq || !d_kp || !d_desc || !d_n || pairs <= 0 || max_n <= 0 || max_q <= 0 ||
        !d_train_match || !d_nmatches || !(max_x > min_x) || !(max_y > min_y))
        return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    return sbp_launch(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, frame_stride_kp, pairs, min_x, min_y,
                      max_x, max_y, th_high, 0, 1, nn_ratio, d_train_match, d_nmatches);
}

// ---------------------------------------------------------------------------- Fuse (search part)
// ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (ORBmatcher.cc:1403-1613, NLeft == -1): the window search of :1499-1570 for
// every projected map point.  The queries do not depend on each other (the Replace / AddObservation bookkeeping of :1572-1595
// is the caller's), so one lane owns one query: it walks the grid columns of its window in GetFeaturesInArea order against
// LDS-resident keypoints AND descriptors (no dependent global gathers inside the lane-serial loop).
// BIG (round 4): keyframes of more than 2900 keypoints (up to 8192: the first two keyframes of a monocular map carry 5 x nFeatures,
// Tracking.cc:210) keep only the grid and the keypoint positions in LDS; descriptors and uRight are read from global memory (L2).
template <bool BIG>
__global__ __launch_bounds__(64) void k_fuse_search(const orbhip_proj_query *q_, const uint8_t *descq_, const int32_t *nq_, int max_q,
                                                    const orbhip_keypoint *kp_, const uint8_t *desc_, const float *uright_,
                                                    const int32_t *n_, int max_n, size_t kp_stride, OrbLevelSigma sig,
                                                    float min_x, float min_y, float max_x, float max_y, int cap_n,
                                                    int32_t *best_idx_, int32_t *best_dist_, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sbp_lds[];
    uint4 *dlds = reinterpret_cast<uint4 *>(sbp_lds);                                 // [cap_n][2]   (BIG: absent)
    uint32_t *cell_start = reinterpret_cast<uint32_t *>(dlds + (BIG ? 0 : 2 * (size_t)cap_n));   // [SBP_CELLS + 1]
    float *kx = reinterpret_cast<float *>(cell_start + SBP_CELLS + 1), *ky = kx + cap_n, *ur = ky + cap_n;      // (BIG: ur absent)
    uint16_t *items = reinterpret_cast<uint16_t *>(BIG ? ky + cap_n : ur + cap_n), *cell_of = items + cap_n, *rank_of = cell_of + cap_n;
    uint8_t *oct = reinterpret_cast<uint8_t *>(rank_of + cap_n);
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int n = n_[pair], nq = nq_[pair];
    const orbhip_proj_query *Q = q_ + (size_t)pair * max_q;
    const uint4 *dQ = reinterpret_cast<const uint4 *>(descq_ + (size_t)pair * max_q * 32);
    const orbhip_keypoint *kp = kp_ + (size_t)pair * kp_stride;
    const uint4 *dT = reinterpret_cast<const uint4 *>(desc_ + (size_t)pair * kp_stride * 32);
    const float *uright = uright_ ? uright_ + (size_t)pair * kp_stride : nullptr;
    int32_t *bi = best_idx_ + (size_t)pair * max_q, *bd = best_dist_ + (size_t)pair * max_q;
    if (n > cap_n || n > max_n || nq > max_q) {
        if (lane == 0) atomicExch(status, ORBHIP_E_CAPACITY);
        for (int t = lane; t < min(nq, max_q); t += 64) { bi[t] = -1; bd[t] = 256; }
        return;
    }
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x));       // Frame.cc:334-335
    const float inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    for (int c = lane; c <= SBP_CELLS; c += 64) cell_start[c] = 0;
    if (!BIG) for (int i = lane; i < n; i += 64) { dlds[2 * i] = dT[2 * i]; dlds[2 * i + 1] = dT[2 * i + 1]; ur[i] = uright ? uright[i] : -1.0f; }
    __syncthreads();
    sbp_build_grid(cell_start, kx, ky, oct, items, cell_of, rank_of, kp, n, min_x, min_y, inv_w, inv_h, lane);
    for (int T = 0; T < nq; T += 64) {
        const int t = T + lane;
        if (t >= nq) continue;
        const orbhip_proj_query qq = Q[t];
        const float x = qq.u, y = qq.v, r = qq.radius;
        int best = 256, besti = -1;
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        if (c0 < SI_COLS && c1 >= 0 && r0 < SI_ROWS && r1 >= 0) {
            const uint4 a0 = dQ[2 * t], a1 = dQ[2 * t + 1];
            for (int cx = c0; cx <= c1; cx++) {
                const int k1 = (int)cell_start[cx * SI_ROWS + r1 + 1];
                for (int k = (int)cell_start[cx * SI_ROWS + r0]; k < k1; k++) {
                    const int idx = items[k];
                    const float dx = __fsub_rn(kx[idx], x), dy = __fsub_rn(ky[idx], y);
                    if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;                                   // Frame.cc:704-708
                    const int lv = oct[idx];
                    if (lv < qq.min_level || lv > qq.max_level) continue;                              // ORBmatcher.cc:1527-1528
                    const float ex = __fsub_rn(x, kx[idx]), ey = __fsub_rn(y, ky[idx]);
                    const float kr = BIG ? (uright ? uright[idx] : -1.0f) : ur[idx];
                    if (kr >= 0) {                                                                      // ORBmatcher.cc:1530-1545
                        const float er = __fsub_rn(qq.ur, kr);
                        const float e2 = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(er, er));
                        if ((double)__fmul_rn(e2, sig.inv_sigma2[lv]) > 7.8) continue;
                    } else {                                                                            // ORBmatcher.cc:1546-1556
                        const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                        if ((double)__fmul_rn(e2, sig.inv_sigma2[lv]) > 5.99) continue;
                    }
                    const int dist = BIG ? hamming256(a0, a1, dT[2 * idx], dT[2 * idx + 1]) : hamming256(a0, a1, dlds[2 * idx], dlds[2 * idx + 1]);
                    if (dist < best) { best = dist; besti = idx; }                                     // ORBmatcher.cc:1564-1568
                }
            }
        }
        bi[t] = besti; bd[t] = best;
    }
}

extern "C" int orbhip_fuse_search_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q, const int32_t *d_nq,
                                         int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *d_u_right,
                                         const int32_t *d_n, int max_n, size_t frame_stride_kp, int pairs,
                                         const float *inv_level_sigma2, int nlevels, float min_x, float min_y, float max_x, float max_y,
                                         int32_t *d_best_idx, int32_t *d_best_dist)
{
    if (!ctx || !d_q || !d_desc_q || !d_nq || !d_kp || !d_desc || !d_n || pairs <= 0 || max_n <= 0 || max_q <= 0 || !inv_level_sigma2 ||
        nlevels < 1 || nlevels > 16 || !d_best_idx || !d_best_dist || !(max_x > min_x) || !(max_y > min_y)) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    OrbLevelSigma sig;
    for (int l = 0; l < 16; l++) sig.inv_sigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.0f;
    // up to 2900 keypoints: keypoints AND descriptors of a keyframe live in LDS (160 KB); beyond (to 8192): positions and grid only
    const bool big = max_n > 2900;
    const int cap_n = ((max_n < (big ? 8192 : 2900) ? max_n : (big ? 8192 : 2900)) + 7) & ~7;
    const size_t lds = (size_t)cap_n * (big ? (4 + 4 + 2 + 2 + 2 + 1) : (32 + 4 + 4 + 4 + 2 + 2 + 2 + 1)) + sizeof(uint32_t) * (SBP_CELLS + 1) + 16;
    if (lds > 160 * 1024 - 512) return ORBHIP_E_BADARG;
    const void *fn = big ? reinterpret_cast<const void *>(k_fuse_search<true>) : reinterpret_cast<const void *>(k_fuse_search<false>);
    if (orb_lds_optin(fn, orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    if (big) hipLaunchKernelGGL(k_fuse_search<true>, dim3(pairs), dim3(64), lds, orbhip_ctx_stream_internal(ctx), d_q, d_desc_q, d_nq, max_q, d_kp, d_desc,
                                d_u_right, d_n, max_n, frame_stride_kp, sig, min_x, min_y, max_x, max_y, cap_n, d_best_idx, d_best_dist,
                                orbhip_ctx_status_internal(ctx));
    else hipLaunchKernelGGL(k_fuse_search<false>, dim3(pairs), dim3(64), lds, orbhip_ctx_stream_internal(ctx), d_q, d_desc_q, d_nq, max_q, d_kp, d_desc,
                            d_u_right, d_n, max_n, frame_stride_kp, sig, min_x, min_y, max_x, max_y, cap_n, d_best_idx, d_best_dist,
                            orbhip_ctx_status_internal(ctx));
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}
