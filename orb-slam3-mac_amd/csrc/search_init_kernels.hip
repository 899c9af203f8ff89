// search_init_kernels.hip -- ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:710-825) over the Frame grid
// (src/Frame.cc:377-408 AssignFeaturesToGrid, :716-726 PosInGrid, :645-714 GetFeaturesInArea): the sequential one-wave-per-pair
// kernel, the replay form in three kernels, the rows form in two, and the vbPrevMatched initialisation.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "frame_grid.h"
#include "match_common.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

// The sequential kernel: one wave per frame pair.  The F1 loop is inherently sequential (vMatchedDistance feeds
// later iterations, ORBmatcher.cc:749), but each iteration's best / second-best search over
// the window's grid cells is order-free except for the tie-break "first candidate in
// GetFeaturesInArea order wins" -- so the 64 lanes scan cells in parallel carrying
// (dist << 23 | visit order) keys and the wave reduces them.
#define SI_MAXN 8192          // keypoints per frame (the monocular-initialisation extractor runs 5 x nFeatures, Tracking.cc:210)
#define SI_CAP0 4096          // octave-0 keypoints per frame held in LDS
#define SI_RANKS 2048         // visit-order key: (cell visit index) * SI_RANKS + rank inside the cell  (3072 cells * 2048 < 2^23)

// Only octave-0 keypoints take part (F1: ORBmatcher.cc:726-728; F2: GetFeaturesInArea(...,level1,level1)
// with level1 == 0), so both frames are first compacted to their octave-0 subsets in LDS.  The grid
// (Frame.cc:377-408) is kept implicitly: each F2 entry carries its cell (round(), Frame.cc:718-719) and
// its rank inside the cell; a keypoint that passes the |dx|<r,|dy|<r test always lies inside the
// floor/ceil cell range of Frame.cc:656-674 (round(a) is within [floor(b), ceil(c)] for b < a < c), so
// scanning the subset and ordering candidates by (cell visit index, rank) reproduces
// GetFeaturesInArea's list exactly.  The F1 loop stays sequential (vMatchedDistance, ORBmatcher.cc:749);
// per F1 point the lanes first collect candidates (LDS only), then evaluate one candidate per lane
// so all descriptor loads are in flight together.
// Register-resident sequential loop of SearchForInitialization (ORBmatcher.cc:726-790) for octave-0 subsets of at most 64 * NS points
// (level 0 holds ~0.22 x nFeatures keypoints: NS = 4 covers 1000 features, NS = 8 covers 2000).  Every lane keeps up to NS F2
// points -- position, grid cell + rank, descriptor, vMatchedDistance, vnMatches21 -- and NS F1 points in registers; F1 point t is
// broadcast from its lane with v_readlane, tests the window predicate on the F2 points directly and takes the Hamming distance:
// no candidate list, no LDS or global access and no barrier inside the chain (the general loop was 60 % candidate scan over
// LDS + 22 % descriptor fetches).  Same keys, same (best, second best), same update rules as the general loop.
template <int NS>
__device__ __forceinline__ int si_register_loop(int lane, int n0, int na0, const float *kx, const float *ky, const uint16_t *cellx, const uint16_t *celly,
                                                const uint16_t *cpos, const uint16_t *gidx, const uint16_t *aidx, uint16_t *bm,
                                                const uint4 *dA, const uint4 *dB, const float *prev, int32_t *m12,
                                                float min_x, float min_y, float inv_w, float inv_h, float r, float nn_ratio)
{
    int nmatches = 0;
    float fkx[NS], fky[NS]; uint32_t fpk[NS]; int fgi[NS], fmd[NS], fm21[NS]; uint4 fd0[NS], fd1[NS];
#pragma unroll
    for (int sl = 0; sl < NS; sl++) {
        const int li = sl * 64 + lane;
        const bool v = li < n0;
        const int lj = v ? li : 0;
        fkx[sl] = kx[lj]; fky[sl] = ky[lj];
        fpk[sl] = v ? ((uint32_t)cellx[lj] | ((uint32_t)celly[lj] << 8) | ((uint32_t)min((int)cpos[lj], SI_RANKS - 1) << 16)) : 0xFFFFu;   // cell (255, 255): never inside a window
        fgi[sl] = v ? (int)gidx[lj] : 0; fmd[sl] = INT_MAX; fm21[sl] = -1;      // (an empty slot must not index the descriptors with LDS garbage)
        fd0[sl] = dB[2 * fgi[sl]]; fd1[sl] = dB[2 * fgi[sl] + 1];
    }
    // the F1 points too: lane l holds points l, l + 64, ... (index, window centre, descriptor); the loop broadcasts point t
    // from its lane with v_readlane, so the sequential chain makes no memory access at all
    int qi[NS]; float qx[NS], qy[NS]; uint4 qd0[NS], qd1[NS];
#pragma unroll
    for (int sl = 0; sl < NS; sl++) {
        const int tq = sl * 64 + lane;
        qi[sl] = tq < na0 ? (int)aidx[tq] : 0;
        qx[sl] = prev[2 * qi[sl]]; qy[sl] = prev[2 * qi[sl] + 1];
        qd0[sl] = dA[2 * qi[sl]]; qd1[sl] = dA[2 * qi[sl] + 1];
    }
    for (int t = 0; t < na0; t++) {
        const int tsl = t >> 6, tln = t & 63;
        int i1 = 0; float x = 0, y = 0; uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
#define SI_RL(v) (uint32_t)__builtin_amdgcn_readlane((int)(v), tln)
#pragma unroll
        for (int sl = 0; sl < NS; sl++)
            if (tsl == sl) {                                            // uniform
                i1 = (int)SI_RL(qi[sl]); x = __uint_as_float(SI_RL(__float_as_uint(qx[sl]))); y = __uint_as_float(SI_RL(__float_as_uint(qy[sl])));
                a0 = make_uint4(SI_RL(qd0[sl].x), SI_RL(qd0[sl].y), SI_RL(qd0[sl].z), SI_RL(qd0[sl].w));
                a1 = make_uint4(SI_RL(qd1[sl].x), SI_RL(qd1[sl].y), SI_RL(qd1[sl].z), SI_RL(qd1[sl].w));
            }
#undef SI_RL
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        if (c0 >= SI_COLS) continue;
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        if (c1 < 0) continue;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        if (r0 >= SI_ROWS) continue;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        if (r1 < 0) continue;
        const int ncy = r1 - r0 + 1;
        // branch-free per slot: window predicate, distance, key (0xFFFFFFFF where the point is no candidate or already matched at
        // a distance <= this one, ORBmatcher.cc:749); per lane the smallest key and the distance of the runner-up
        uint32_t lk1 = 0xFFFFFFFFu, ld2 = 0xFFFFFFFFu; int best_sl = 0;
        const uint32_t cw = (uint32_t)(c1 - c0), rh = (uint32_t)(r1 - r0);
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            if (sl * 64 >= n0) break;                                   // uniform
            const uint32_t dcx = (fpk[sl] & 255u) - (uint32_t)c0, dcy = ((fpk[sl] >> 8) & 255u) - (uint32_t)r0;
            const int dist = hamming256(a0, a1, fd0[sl], fd1[sl]);
            const bool c = dcx <= cw && dcy <= rh && fabsf(__fsub_rn(fkx[sl], x)) < r && fabsf(__fsub_rn(fky[sl], y)) < r && !(fmd[sl] <= dist);
            const uint32_t key = c ? ((uint32_t)dist << 23) | ((dcx * (uint32_t)ncy + dcy) * SI_RANKS + (fpk[sl] >> 16)) : 0xFFFFFFFFu;
            ld2 = min(ld2, max(lk1, key));                              // the larger of (best so far, new) is a runner-up
            best_sl = key < lk1 ? sl : best_sl;
            lk1 = min(lk1, key);
        }
        const uint32_t k1 = wave_min_u32_dpp(lk1);
        // second best over the wave: every lane's runner-up, and the best of every lane that is not the winner (keys are unique)
        const uint32_t k2 = wave_min_u32_dpp(lk1 == k1 ? ld2 : lk1);
        const int d2 = k2 == 0xFFFFFFFFu ? INT_MAX : (int)(k2 >> 23);
        if (k1 == 0xFFFFFFFFu) continue;                                // no candidate, or none below its vMatchedDistance
        const int best = (int)(k1 >> 23);
        if (!(best <= TH_LOW && (float)best < __fmul_rn((float)d2, nn_ratio))) continue;   // ORBmatcher.cc:764-766
        const unsigned long long owner = __ballot(lk1 == k1);          // keys are unique: exactly one lane
        const int ol = __builtin_amdgcn_readfirstlane(__ffsll((long long)owner) - 1);
        const int bsl = __builtin_amdgcn_readlane(best_sl, ol);
        int old = -1, best_idx = 0;
#pragma unroll
        for (int sl = 0; sl < NS; sl++)
            if (bsl == sl) {                                            // uniform
                old = __builtin_amdgcn_readlane(fm21[sl], ol); best_idx = __builtin_amdgcn_readlane(fgi[sl], ol);
                if (lane == ol) { fm21[sl] = i1; fmd[sl] = best; }
            }
        if (old >= 0) nmatches--;                                       // ORBmatcher.cc:768-772
        nmatches++;
        if (lane == 0) {
            if (old >= 0) m12[old] = -1;
            m12[i1] = best_idx;
            bm[i1] = (uint16_t)best_idx;                                // its rotation-histogram entry is made after the loop
        }
    }
    return nmatches;
}

// Tail of SearchForInitialization shared by both forms: rotation consistency (ORBmatcher.cc:792-815, 2307-2348) and the vbPrevMatched
// update (:818-822).  bm[i1] = the F2 index an F1 keypoint was matched to at some time (0xFFFF: never); returns nmatches (lane 0's value counts).
__device__ __forceinline__ int si_tail(int lane, int n1, const orbhip_keypoint *kpA, const orbhip_keypoint *kpB, const uint16_t *bm, int8_t *bin_of,
                                       int *hist, int *s_keep, int32_t *m12, float *prev, int nmatches, int check_ori)
{
    __syncthreads();
    // Every F1 point that was matched at some time has one histogram entry (ORBmatcher.cc:778-789), also when it was displaced later.
    if (check_ori) {
        for (int i1 = lane; i1 < n1; i1 += 64) {
            const int b = bm[i1];
            if (b == 0xFFFF) continue;
            const int bin = rot_bin(kpA[i1].angle, kpB[b].angle);
            atomicAdd(&hist[bin], 1); bin_of[i1] = (int8_t)bin;
        }
        __syncthreads();
        if (lane == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        int removed = 0;
        for (int i1 = lane; i1 < n1; i1 += 64) {
            const int b = bin_of[i1];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            if (m12[i1] >= 0) { m12[i1] = -1; removed++; }
        }
        removed = wave_sum_dpp(removed);
        nmatches -= removed;                                                // lane 0's copy is the one written out
    }
    __syncthreads();
    for (int i1 = lane; i1 < n1; i1 += 64)                                  // ORBmatcher.cc:818-822
        if (m12[i1] >= 0) { prev[2 * i1] = kpB[m12[i1]].x; prev[2 * i1 + 1] = kpB[m12[i1]].y; }
    return nmatches;
}

#ifdef SI_PROF
__device__ long long g_si_prof[8];            // debug build only (EXTRA=-DSI_PROF): cycles of setup / candidate scan / distances + reduction / update / tail, iterations
#define SI_T(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const long long t_ = clock64(); g_si_prof[i] += t_ - t_prev; t_prev = t_; } } while (0)
extern "C" int orbhip_debug_si_prof(long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_si_prof), 64) != hipSuccess) return ORBHIP_E_HIP;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_si_prof), z, 64) != hipSuccess) return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
#else
#define SI_T(i) do { } while (0)
#endif
__global__ __launch_bounds__(64) void k_search_init(const orbhip_keypoint *kpA_, const uint8_t *descA_, const int32_t *nA,
                                                    const orbhip_keypoint *kpB_, const uint8_t *descB_, const int32_t *nB,
                                                    int max_n, size_t kp_stride, float min_x, float min_y, float max_x, float max_y,
                                                    int window, float nn_ratio, int check_ori, int cap0, int maxn,
                                                    float *prev_, int32_t *m12_, int32_t *nmatches_, int32_t *status, const int32_t *redo_,
                                                    int32_t *redo_out)
{
    // redo_: only the flagged pairs are done (the others were finished by the replay form, or by the small-LDS launch of this kernel);
    // redo_out: this launch carves its LDS for cap0 octave-0 points only -- a pair with more is flagged there and left to the next launch
    if (redo_ && !redo_[blockIdx.x]) { if (redo_out && threadIdx.x == 0) redo_out[blockIdx.x] = 0; return; }
    // dynamic LDS, carved by the launcher's capacities: cap0 octave-0 entries per frame, maxn keypoints per frame
    extern __shared__ __attribute__((aligned(16))) uint8_t si_lds[];
    float *kx = reinterpret_cast<float *>(si_lds), *ky = kx + cap0;
    int *matched_dist = reinterpret_cast<int *>(ky + cap0);
    uint32_t *cand_key = reinterpret_cast<uint32_t *>(matched_dist + cap0);
    uint16_t *cellx = reinterpret_cast<uint16_t *>(cand_key + cap0), *celly = cellx + cap0, *cpos = celly + cap0, *gidx = cpos + cap0;
    int16_t *m21 = reinterpret_cast<int16_t *>(gidx + cap0);
    uint16_t *aidx = reinterpret_cast<uint16_t *>(m21 + cap0), *cand_li = aidx + cap0;
    uint16_t *bm = cand_li + cap0;                                  // [maxn] F2 index an F1 keypoint was matched to (0xFFFF = never)
    int8_t *bin_of = reinterpret_cast<int8_t *>(bm + maxn);
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
#ifdef SI_PROF
    long long t_prev = clock64();
#endif
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const int n1 = nA[pair], n2 = nB[pair];
    const orbhip_keypoint *kpA = kpA_ + (size_t)pair * kp_stride, *kpB = kpB_ + (size_t)pair * kp_stride;
    const uint4 *dA = reinterpret_cast<const uint4 *>(descA_ + (size_t)pair * kp_stride * 32);
    const uint4 *dB = reinterpret_cast<const uint4 *>(descB_ + (size_t)pair * kp_stride * 32);
    float *prev = prev_ + (size_t)pair * max_n * 2;
    int32_t *m12 = m12_ + (size_t)pair * max_n;
    if (n1 > maxn || n2 > maxn) {                                    // (nothing left for a second launch: it would report the same)
        if (lane == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; if (redo_out) redo_out[pair] = 0; }
        return;
    }
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x));       // Frame.cc:334-335
    const float inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    // ---- octave-0 subset of F2 that PosInGrid accepts, index order kept (= insertion order of the grid)
    int n0 = 0;
    for (int i0 = 0; i0 < n2; i0 += 64) {
        const int i = i0 + lane;
        bool in = false; int px = 0, py = 0; float fx = 0, fy = 0;
        if (i < n2) {
            const orbhip_keypoint k = kpB[i];
            fx = k.x; fy = k.y;
            px = (int)roundf(__fmul_rn(__fsub_rn(fx, min_x), inv_w));             // round(), Frame.cc:718-719
            py = (int)roundf(__fmul_rn(__fsub_rn(fy, min_y), inv_h));
            in = k.octave == 0 && px >= 0 && px < SI_COLS && py >= 0 && py < SI_ROWS;
        }
        const unsigned long long bal = __ballot(in);
        const int li = n0 + __popcll(bal & lt_mask);
        if (in && li < cap0) {
            kx[li] = fx; ky[li] = fy; cellx[li] = (uint16_t)px; celly[li] = (uint16_t)py; gidx[li] = (uint16_t)i;
            matched_dist[li] = INT_MAX; m21[li] = -1;
        }
        n0 += __popcll(bal);
    }
    // ---- octave-0 subset of F1 (ORBmatcher.cc:726-728)
    int na0 = 0;
    for (int i0 = 0; i0 < n1; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n1 && kpA[i].octave == 0;
        const unsigned long long bal = __ballot(in);
        const int li = na0 + __popcll(bal & lt_mask);
        if (in && li < cap0) aidx[li] = (uint16_t)i;
        na0 += __popcll(bal);
        if (i < n1) { m12[i] = -1; bin_of[i] = -1; bm[i] = 0xFFFFu; }
    }
    if (redo_out) {
        if (lane == 0) redo_out[pair] = (n0 > cap0 || na0 > cap0) ? 1 : 0;
        if (n0 > cap0 || na0 > cap0) return;                                    // (m12 was reset, prev is untouched: the next launch starts over)
    }
    if (n0 > cap0 || na0 > cap0) { if (lane == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; } return; }
    __syncthreads();
    for (int li = lane; li < n0; li += 64) {                                    // rank inside the grid cell
        const int cx = cellx[li], cy = celly[li];
        int rank = 0;
        for (int j = 0; j < li; j++) rank += (cellx[j] == cx && celly[j] == cy);
        cpos[li] = (uint16_t)rank;
    }
    __syncthreads();
    SI_T(0);
    // ---- sequential F1 loop
    int nmatches = 0;
    const float r = (float)window;
    if (n0 <= 4 * 64 && na0 <= 4 * 64)
        nmatches = si_register_loop<4>(lane, n0, na0, kx, ky, cellx, celly, cpos, gidx, aidx, bm, dA, dB, prev, m12, min_x, min_y, inv_w, inv_h, r, nn_ratio);
    else if (n0 <= 8 * 64 && na0 <= 8 * 64)
        nmatches = si_register_loop<8>(lane, n0, na0, kx, ky, cellx, celly, cpos, gidx, aidx, bm, dA, dB, prev, m12, min_x, min_y, inv_w, inv_h, r, nn_ratio);
    else {
    // the next F1 point's window centre and descriptor are fetched one iteration ahead
    int i1n = na0 > 0 ? (int)aidx[0] : 0;
    float xn = 0, yn = 0; uint4 pd0 = make_uint4(0, 0, 0, 0), pd1 = pd0;
    if (na0 > 0) { xn = prev[2 * i1n]; yn = prev[2 * i1n + 1]; pd0 = dA[2 * i1n]; pd1 = dA[2 * i1n + 1]; }
    for (int t = 0; t < na0; t++) {
        const int i1 = i1n;
        const float x = xn, y = yn;
        const uint4 a0 = pd0, a1 = pd1;
        if (t + 1 < na0) { i1n = aidx[t + 1]; xn = prev[2 * i1n]; yn = prev[2 * i1n + 1]; pd0 = dA[2 * i1n]; pd1 = dA[2 * i1n + 1]; }
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        if (c0 >= SI_COLS) continue;
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        if (c1 < 0) continue;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        if (r0 >= SI_ROWS) continue;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        if (r1 < 0) continue;
        const int ncy = r1 - r0 + 1;
        // phase A: collect candidates (GetFeaturesInArea's result set, any order, with their visit-order key)
        int ncand = 0;
        for (int l0 = 0; l0 < n0; l0 += 64) {
            const int li = l0 + lane;
            bool c = false; uint32_t key = 0;
            if (li < n0) {
                const int cx = cellx[li], cy = celly[li];
                c = cx >= c0 && cx <= c1 && cy >= r0 && cy <= r1 &&
                    fabsf(__fsub_rn(kx[li], x)) < r && fabsf(__fsub_rn(ky[li], y)) < r;
                key = (uint32_t)(((cx - c0) * ncy + (cy - r0)) * SI_RANKS + min((int)cpos[li], SI_RANKS - 1));
            }
            const unsigned long long bal = __ballot(c);
            if (c) { const int o = ncand + __popcll(bal & lt_mask); cand_li[o] = (uint16_t)li; cand_key[o] = key; }
            ncand += __popcll(bal);
        }
        SI_T(1);
        if (ncand == 0) continue;                                           // vIndices2.empty(), ORBmatcher.cc:732-733
        __syncthreads();
        // phase B: one candidate per lane
        uint32_t lk1 = 0xFFFFFFFFu; int d2 = INT_MAX, best_li = -1;
        for (int q0 = 0; q0 < ncand; q0 += 64) {
            const int q = q0 + lane;
            if (q < ncand) {
                const int li = cand_li[q];
                const int i2 = gidx[li];
                const int dist = hamming256(a0, a1, dB[2 * i2], dB[2 * i2 + 1]);
                if (!(matched_dist[li] <= dist)) {                          // ORBmatcher.cc:749
                    const uint32_t key = ((uint32_t)dist << 23) | cand_key[q];
                    if (key < lk1) { if (lk1 != 0xFFFFFFFFu) d2 = min(d2, (int)(lk1 >> 23)); lk1 = key; best_li = li; }
                    else d2 = min(d2, dist);
                }
            }
        }
        uint32_t k1 = lk1;
        // (best key, second-best distance) over the wave on the DPP path (scan order; the operation is associative and commutative)
#define SI_STEP(CTRL, RM) do { const uint32_t ok1 = (uint32_t)dpp_mov<CTRL, RM>(-1, (int)k1); const int od2 = dpp_mov<CTRL, RM>(INT_MAX, d2); \
            const uint32_t lose = max(k1, ok1); d2 = min(min(d2, od2), lose == 0xFFFFFFFFu ? INT_MAX : (int)(lose >> 23)); k1 = min(k1, ok1); } while (0)
        SI_STEP(ORB_DPP_ROW_SHR(1), 0xF); SI_STEP(ORB_DPP_ROW_SHR(2), 0xF); SI_STEP(ORB_DPP_ROW_SHR(4), 0xF); SI_STEP(ORB_DPP_ROW_SHR(8), 0xF);
        SI_STEP(ORB_DPP_ROW_BCAST15, 0xA); SI_STEP(ORB_DPP_ROW_BCAST31, 0xC);
#undef SI_STEP
        k1 = (uint32_t)__builtin_amdgcn_readlane((int)k1, 63); d2 = __builtin_amdgcn_readlane(d2, 63);
        __syncthreads();                                                    // cand_* reused by the next F1 point
        SI_T(2);
#ifdef SI_PROF
        if (blockIdx.x == 0 && threadIdx.x == 0) { g_si_prof[5] += 1; g_si_prof[6] += ncand; }
#endif
        if (k1 == 0xFFFFFFFFu) continue;                                    // bestDist stays INT_MAX > TH_LOW
        const int best = (int)(k1 >> 23);
        if (!(best <= TH_LOW && (float)best < __fmul_rn((float)d2, nn_ratio))) continue;   // ORBmatcher.cc:764-766
        const unsigned long long owner = __ballot(lk1 == k1);              // keys are unique: exactly one lane
        const int bli = __builtin_amdgcn_readlane(best_li, __builtin_amdgcn_readfirstlane(__ffsll((long long)owner) - 1));
        if (lane == 0) {
            const int best_idx = gidx[bli];
            const int old = m21[bli];
            if (old >= 0) { m12[old] = -1; nmatches--; }                    // ORBmatcher.cc:768-772
            m12[i1] = best_idx; m21[bli] = (int16_t)i1; matched_dist[bli] = best; nmatches++;
            bm[i1] = (uint16_t)best_idx;                                    // its rotation-histogram entry is made after the loop
        }
        __syncthreads();
        SI_T(3);
    }
    }
    nmatches = si_tail(lane, n1, kpA, kpB, bm, bin_of, hist, s_keep, m12, prev, nmatches, check_ori);
    if (lane == 0) nmatches_[pair] = nmatches;
    SI_T(4);
}

// ---------------------------------------------------------------------------------------------------------------------
// Replay form of SearchForInitialization (round 3).  The F1 loop is sequential only through vMatchedDistance
// (ORBmatcher.cc:749): a candidate is skipped when its F2 point already holds a match at a distance <= this one.  Which F2 points lie
// in a query's window, their Hamming distances and GetFeaturesInArea's visiting order do not depend on it.  So:
//   k_si_prep        one wave per pair: the octave-0 subsets of both frames (the only points that take part) written out compactly --
//                    F2: position, grid cell + rank inside the cell, frame index, descriptor; F1: frame indices;
//   k_si_candidates  ONE WAVE PER F1 POINT over the whole chip: every F2 subset point is tested against the window, keys
//                    distance << 23 | visit order (the sequential kernels' key) are ranked by counting and the SIL_K smallest stored with
//                    their subset positions (transposed: lane = query of a 64-query trip);
//   k_si_replay      one wave per pair, 64 queries per trip: a lane's best / second best are the first two list entries NOT skipped by
//                    the current vMatchedDistance -- it only ever decreases, so a skipped entry stays skipped and a cursor only moves forward.
//                    Lanes speculate; an accepting lane publishes its F2 point (LDS atomicMin of the lane id); the prefix of lanes up to the
//                    first one whose best or second best an earlier lane of the round wants becomes final and applies its updates
//                    (distinct F2 points inside a prefix by construction), the rest look again.
// Same candidates, same keys, same update rule as k_search_init; both run in every test (si_form fixture).  A pair whose subsets exceed the
// work area, or a query whose truncated list runs dry before a best AND a second best were found, is flagged on the device and done by
// k_search_init, which returns at once for the others.
#define SIL_K 64                   // list entries kept per query
#define SIL_BUF 512                // candidates a query may have before its pair falls back
#define SIL_CAP 1024               // octave-0 points per frame the replay form handles
struct SiWork {
    int cap0, chunks;
    float4 *rec;                   // [pairs][cap0]  F2 octave-0 subset: x, y, bits(cell x | cell y << 8 | rank << 16), bits(frame index)
    uint4 *desc;                   // [pairs][cap0][2]
    uint16_t *aidx;                // [pairs][cap0]  F1 octave-0 subset -> frame index
    int32_t *n0, *na0;             // [pairs]
    uint32_t *lkey;                // [pairs][chunks][SIL_K][64]
    uint16_t *lli;                 // [pairs][chunks][SIL_K][64]
    int32_t *count;                // [pairs][cap0]  candidates of the query (may exceed SIL_K; INT_MAX: more than SIL_BUF)
    int32_t *redo;                 // [pairs]
};

__global__ __launch_bounds__(64) void k_si_prep(const orbhip_keypoint *kpA_, const int32_t *nA, const orbhip_keypoint *kpB_, const uint8_t *descB_, const int32_t *nB,
                                                size_t kp_stride, float min_x, float min_y, float max_x, float max_y, int maxn, SiWork W)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sip_lds[];
    uint16_t *cellx = reinterpret_cast<uint16_t *>(sip_lds), *celly = cellx + W.cap0, *gidx = celly + W.cap0;
    const int pair = blockIdx.x, lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const int n1 = nA[pair], n2 = nB[pair];
    const orbhip_keypoint *kpA = kpA_ + (size_t)pair * kp_stride, *kpB = kpB_ + (size_t)pair * kp_stride;
    const uint4 *dB = reinterpret_cast<const uint4 *>(descB_ + (size_t)pair * kp_stride * 32);
    if (lane == 0) W.redo[pair] = 0;
    if (n1 > maxn || n2 > maxn) { if (lane == 0) W.redo[pair] = 1; return; }       // (k_search_init reports the capacity error)
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x)), inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    float4 *rec = W.rec + (size_t)pair * W.cap0;
    uint4 *desc = W.desc + (size_t)pair * W.cap0 * 2;
    uint16_t *aidx = W.aidx + (size_t)pair * W.cap0;
    int n0 = 0;                                                                    // F2: octave 0 and inside the grid, index order kept
    for (int i0 = 0; i0 < n2; i0 += 256) {                                         // four chunks of loads in flight (the loop is a chain of global round trips otherwise)
        float fxs[4], fys[4]; int ocs[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = min(i0 + 64 * u + lane, n2 - 1);
            fxs[u] = kpB[i].x; fys[u] = kpB[i].y; ocs[u] = kpB[i].octave;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + 64 * u + lane;
            const float fx = fxs[u], fy = fys[u];
            const int px = (int)roundf(__fmul_rn(__fsub_rn(fx, min_x), inv_w)), py = (int)roundf(__fmul_rn(__fsub_rn(fy, min_y), inv_h));      // Frame.cc:718-719
            const bool in = i < n2 && ocs[u] == 0 && px >= 0 && px < SI_COLS && py >= 0 && py < SI_ROWS;
            const unsigned long long bal = __ballot(in);
            const int li = n0 + __popcll(bal & lt_mask);
            if (in && li < W.cap0) {
                cellx[li] = (uint16_t)px; celly[li] = (uint16_t)py; gidx[li] = (uint16_t)i;
                rec[li] = make_float4(fx, fy, 0.0f, __uint_as_float((uint32_t)i));
                desc[2 * li] = dB[2 * i]; desc[2 * li + 1] = dB[2 * i + 1];
            }
            n0 += __popcll(bal);
        }
    }
    int na0 = 0;                                                                   // F1: octave 0 (ORBmatcher.cc:726-728)
    for (int i0 = 0; i0 < n1; i0 += 256) {
        int ocs[4];
#pragma unroll
        for (int u = 0; u < 4; u++) ocs[u] = kpA[min(i0 + 64 * u + lane, n1 - 1)].octave;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + 64 * u + lane;
            const bool in = i < n1 && ocs[u] == 0;
            const unsigned long long bal = __ballot(in);
            const int li = na0 + __popcll(bal & lt_mask);
            if (in && li < W.cap0) aidx[li] = (uint16_t)i;
            na0 += __popcll(bal);
        }
    }
    if (lane == 0) { W.n0[pair] = n0; W.na0[pair] = na0; }
    if (n0 > W.cap0 || na0 > W.cap0) { if (lane == 0) W.redo[pair] = 1; return; }
    __syncthreads();
    for (int li = lane; li < n0; li += 64) {                                       // rank inside the grid cell = position in the cell's vector
        const int cx = cellx[li], cy = celly[li];
        int rank = 0;
        for (int j = 0; j < li; j++) rank += (cellx[j] == cx && celly[j] == cy);
        reinterpret_cast<uint32_t *>(rec + li)[2] = (uint32_t)cx | ((uint32_t)cy << 8) | ((uint32_t)min(rank, SI_RANKS - 1) << 16);
    }
}

__global__ __launch_bounds__(256) void k_si_candidates(const uint8_t *descA_, size_t kp_stride, int max_n, const float *prev_, float min_x, float min_y,
                                                       float max_x, float max_y, int window, SiWork W)
{
    __shared__ uint32_t kbuf_all[4][SIL_BUF];
    __shared__ uint16_t lbuf_all[4][SIL_BUF];
    const int pair = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + w;
    if (W.redo[pair]) return;
    const int n0 = W.n0[pair], na0 = W.na0[pair];
    if (t >= na0) return;
    uint32_t *kbuf = kbuf_all[w]; uint16_t *lbuf = lbuf_all[w];
    const int i1 = W.aidx[(size_t)pair * W.cap0 + t];
    const uint4 *dA = reinterpret_cast<const uint4 *>(descA_ + ((size_t)pair * kp_stride + i1) * 32);
    const uint4 a0 = dA[0], a1 = dA[1];
    const float x = prev_[((size_t)pair * max_n + i1) * 2], y = prev_[((size_t)pair * max_n + i1) * 2 + 1], r = (float)window;
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x)), inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    int32_t *count = W.count + (size_t)pair * W.cap0;
    int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;                   // Frame.cc:656-674
    int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
    int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
    int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
    if (c0 >= SI_COLS || c1 < 0 || r0 >= SI_ROWS || r1 < 0) { if (lane == 0) count[t] = 0; return; }
    const uint32_t cw = (uint32_t)(c1 - c0), rh = (uint32_t)(r1 - r0), ncy = rh + 1;
    const float4 *rec = W.rec + (size_t)pair * W.cap0;
    const uint4 *dC = W.desc + (size_t)pair * W.cap0 * 2;
    int total = 0;
    for (int l0 = 0; l0 < n0; l0 += 64) {
        const int li = l0 + lane;
        bool ok = li < n0;
        uint32_t key = 0xFFFFFFFFu;
        if (ok) {
            const float4 k = rec[li];
            const uint32_t bits = __float_as_uint(k.z);
            const uint32_t dcx = (bits & 255u) - (uint32_t)c0, dcy = ((bits >> 8) & 255u) - (uint32_t)r0;
            ok = dcx <= cw && dcy <= rh && fabsf(__fsub_rn(k.x, x)) < r && fabsf(__fsub_rn(k.y, y)) < r;
            if (ok) key = ((uint32_t)hamming256(a0, a1, dC[2 * li], dC[2 * li + 1]) << 23) | ((dcx * ncy + dcy) * SI_RANKS + (bits >> 16));
        }
        const unsigned long long m = __ballot(ok);
        const int before = __popcll(m & ((1ull << lane) - 1));
        if (ok && total + before < SIL_BUF) { kbuf[total + before] = key; lbuf[total + before] = (uint16_t)li; }
        total += __popcll(m);
    }
    if (total > SIL_BUF) { if (lane == 0) count[t] = 0x7FFFFFFF; return; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const size_t lo = (((size_t)pair * W.chunks + (t >> 6)) * SIL_K) * 64 + (t & 63);
    for (int e = lane; e < total; e += 64) {                                       // rank by counting (keys are unique)
        const uint32_t mine = kbuf[e];
        int rank = 0;
        for (int j = 0; j < total; j++) rank += kbuf[j] < mine;
        if (rank < SIL_K) { W.lkey[lo + (size_t)rank * 64] = mine; W.lli[lo + (size_t)rank * 64] = lbuf[e]; }
    }
    if (lane == 0) count[t] = total;
}

__global__ __launch_bounds__(64) void k_si_replay(const orbhip_keypoint *kpA_, const int32_t *nA, const orbhip_keypoint *kpB_, size_t kp_stride, int max_n,
                                                  float nn_ratio, int check_ori, int maxn, SiWork W, float *prev_, int32_t *m12_, int32_t *nmatches_)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sir_lds[];
    int *md = reinterpret_cast<int *>(sir_lds);                          // [cap0] vMatchedDistance of the F2 subset
    int *m21 = md + W.cap0;                                               // [cap0] vnMatches21
    int *owner = m21 + W.cap0;                                            // [cap0] lowest lane of this round that wants the point (64: none)
    uint32_t *tkey = reinterpret_cast<uint32_t *>(owner + W.cap0);        // [SIL_K][64] this trip's lists
    uint16_t *tli = reinterpret_cast<uint16_t *>(tkey + SIL_K * 64);      // [SIL_K][64]
    uint16_t *bm = tli + SIL_K * 64;                                      // [maxn]
    int8_t *bin_of = reinterpret_cast<int8_t *>(bm + maxn);               // [maxn]
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (W.redo[pair]) return;
    const int n1 = nA[pair], n0 = W.n0[pair], na0 = W.na0[pair];
    const orbhip_keypoint *kpA = kpA_ + (size_t)pair * kp_stride, *kpB = kpB_ + (size_t)pair * kp_stride;
    float *prev = prev_ + (size_t)pair * max_n * 2;
    int32_t *m12 = m12_ + (size_t)pair * max_n;
    const int32_t *count = W.count + (size_t)pair * W.cap0;
    const uint16_t *aidx = W.aidx + (size_t)pair * W.cap0;
    const float4 *rec = W.rec + (size_t)pair * W.cap0;
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    for (int i = lane; i < n0; i += 64) { md[i] = INT_MAX; m21[i] = -1; owner[i] = 64; }
    for (int i = lane; i < n1; i += 64) { m12[i] = -1; bin_of[i] = -1; bm[i] = 0xFFFFu; }
    __syncthreads();
    int nmatches = 0;
    bool give_up = false;
    for (int t0 = 0; t0 < na0 && !give_up; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < na0;
        const int cnt_all = valid ? count[t] : 0;
        if (__ballot(cnt_all == 0x7FFFFFFF)) { give_up = true; break; }
        const int cnt = min(cnt_all, SIL_K);
        const int i1 = valid ? (int)aidx[t] : 0;
        // this trip's lists into LDS, coalesced (entry j of all 64 queries is one 256-byte row)
        const int maxcnt = wave_max_dpp(cnt);
        const size_t lo = (((size_t)pair * W.chunks + (t0 >> 6)) * SIL_K) * 64 + lane;
        for (int j = 0; j < maxcnt; j++) { tkey[j * 64 + lane] = W.lkey[lo + (size_t)j * 64]; tli[j * 64 + lane] = W.lli[lo + (size_t)j * 64]; }
        __syncthreads();
        int ptr = 0;
        bool fin = !valid || cnt == 0;
        while (true) {
            uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
            int l1 = 0, l2 = 0;
            bool accept = false, starved = false;
            if (!fin) {
                while (ptr < cnt) { const uint32_t k = tkey[ptr * 64 + lane]; const int li = tli[ptr * 64 + lane]; if (!(md[li] <= (int)(k >> 23))) { k1 = k; l1 = li; break; } ptr++; }   // ORBmatcher.cc:749
                if (k1 == 0xFFFFFFFFu) starved = cnt_all > SIL_K;                  // ran out of a truncated list
                else {
                    int p2 = ptr + 1;
                    while (p2 < cnt) { const uint32_t k = tkey[p2 * 64 + lane]; const int li = tli[p2 * 64 + lane]; if (!(md[li] <= (int)(k >> 23))) { k2 = k; l2 = li; break; } p2++; }
                    if (k2 == 0xFFFFFFFFu && cnt_all > SIL_K) starved = true;
                    const int best = (int)(k1 >> 23), d2 = k2 == 0xFFFFFFFFu ? INT_MAX : (int)(k2 >> 23);
                    accept = best <= TH_LOW && (float)best < __fmul_rn((float)d2, nn_ratio);          // ORBmatcher.cc:764-766
                }
            }
            if (__ballot(starved)) { give_up = true; break; }
            if (!fin && accept) atomicMin(&owner[l1], lane);
            __syncthreads();
            bool conflict = false;
            if (!fin) {
                if (k1 != 0xFFFFFFFFu) conflict = owner[l1] < lane;
                if (k2 != 0xFFFFFFFFu) conflict = conflict || owner[l2] < lane;
            }
            const unsigned long long cm = __ballot(conflict);
            const int f = cm ? __ffsll((long long)cm) - 1 : 64;                    // lanes below f are final
            __syncthreads();
            if (!fin && accept) owner[l1] = 64;
            if (!fin && lane < f) {
                if (accept) {                                                      // ORBmatcher.cc:766-790
                    const int old = m21[l1];
                    const int best_idx = (int)__float_as_uint(rec[l1].w);
                    if (old >= 0) { m12[old] = -1; nmatches--; }
                    m12[i1] = best_idx; m21[l1] = i1; md[l1] = (int)(k1 >> 23); nmatches++;
                    bm[i1] = (uint16_t)best_idx;
                }
                fin = true;
            }
            __syncthreads();
            if (f == 64) break;
        }
    }
    if (give_up) { if (lane == 0) W.redo[pair] = 1; return; }                      // k_search_init starts over (it resets m12; prev is untouched so far)
    nmatches = wave_sum_dpp(nmatches);
    nmatches = si_tail(lane, n1, kpA, kpB, bm, bin_of, hist, s_keep, m12, prev, nmatches, check_ori);
    if (lane == 0) nmatches_[pair] = nmatches;
}

// ---------------------------------------------------------------------------------------------------------------------
// Rows form of SearchForInitialization (round 8).  si_register_loop pays the state-free work -- window cell range, descriptor broadcast,
// Hamming distance, position and cell tests, visiting-order key -- on the one-wave chain, once per F1 point.  Here a throughput kernel
// does all of it for every (F1, F2) octave-0 combination of a pair and the chain only applies the vMatchedDistance rule:
//   k_si_rows    one 256-thread workgroup per pair: both octave-0 subsets compacted into LDS (k_search_init's predicates), the visiting
//                order ord[j] of every F2 subset point, and one uint16_t per (F1 point t, F2 point j): the Hamming distance where j
//                passes t's window test (si_register_loop's, without its fmd term), 0xFFFF where not;
//   k_si_chain   one wave per pair: per F1 point one 8- or 16-byte load per lane (its row share, fetched SIR_PF - 1 points ahead),
//                per slot the vMatchedDistance test and the key, one joint DPP pass for (best, second best), then the acceptance test
//                and the owner update of si_register_loop, and si_tail.
// The visiting order: si_register_loop's key carries ((cx - c0) * ncy + (cy - r0)) * SI_RANKS + rank in its low 23 bits.  For two
// candidates of the SAME query that compares exactly like (cx, cy, rank), because cy - r0 < ncy, and the rank inside a cell is subset-index
// order.  ord[j] = the number of subset points ahead of j in (cell x, cell y, subset index) order is strictly monotone in that triple and
// does not depend on the query.  The keys are used only through min, equality and >> 23, so dist << 23 | ord[j] picks the same winner and
// the same second-best distance.  (ord < 512 and no rank reaches SI_RANKS - 1 here, so the clamp of the old key never acts.)
// Row t of a pair's matrix holds, for lane l, the NS slots j = sl * 64 + l side by side (NS = 4 up to 256 F2 subset points, else 8): a lane
// fetches its share with one load and the wave reads one contiguous block of 64 * NS * 2 bytes.  uint16_t, not a clamped uint8_t: a
// dropped second best at distance 255 or 256 would change best < d2 * ratio for a small nn_ratio.
// Pairs with more than SIR_CAP octave-0 points in either frame, or with n1 / n2 above maxn, are flagged in `redo` and done by
// k_search_init, which also reports the capacity error.
#define SIR_CAP 512                // octave-0 points per frame the rows form handles (the NS = 8 tier)
#define SIR_PF 8                   // the chain's ring of row shares: loads run SIR_PF - 1 F1 points ahead (the rows are state-free: any distance is legal)
struct SiRows {
    int cap, cols;                 // rows and uint16_t columns allocated per pair (cols: 256 or 512)
    uint16_t *mat;                 // [pairs][cap * cols]  row t of a pair at t * 64 * NS
    uint16_t *aidx;                // [pairs][SIR_CAP]     F1 octave-0 subset -> frame index
    uint32_t *frec;                // [pairs][SIR_CAP]     F2 octave-0 subset: ord | frame index << 16
    int32_t *n0, *na0, *redo;      // [pairs]
};
template <int NS> struct alignas(NS * 2) SiRowShare { uint32_t w[NS / 2]; };      // a lane's NS distances of one row

// the 256 threads' share of one compaction step: position of this thread's element among the accepted ones, and their total
__device__ __forceinline__ int si_rows_slot(bool in, int lane, int w, int *wcnt, int &total)
{
    const unsigned long long bal = __ballot(in);
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int base = total;
#pragma unroll
    for (int ww = 0; ww < 4; ww++) { const int c = wcnt[ww]; base += ww < w ? c : 0; total += c; }
    return base + __popcll(bal & ((1ull << lane) - 1));
}

// Four slots (sl0 .. sl0 + 3) of every row of a pair whose rows hold NS slots per lane: the F2 points of the four slots stay in registers,
// a wave takes every fourth row.  (NS = 8 in two passes: eight slots at once need 187 registers, two workgroups per CU; four need
// fewer than 128, and all 1023 workgroups of the bench's batch are resident at once.)
template <int NS>
__device__ __forceinline__ void si_rows_fill(int sl0, int lane, int w, int n0, int na0, const float *fx, const float *fy, const uint16_t *fcx, const uint16_t *fcy,
                                             const uint16_t *gidx, const float *qx, const float *qy, const uint4 *qd, const uint4 *dB, uint16_t *mat,
                                             float min_x, float min_y, float inv_w, float inv_h, float r)
{
    float kx[4], ky[4]; uint32_t cx[4], cy[4]; uint4 d0[4], d1[4];
#pragma unroll
    for (int sl = 0; sl < 4; sl++) {
        const int li = (sl0 + sl) * 64 + lane;
        const bool v = li < n0;
        const int lj = v ? li : 0;
        kx[sl] = fx[lj]; ky[sl] = fy[lj];
        cx[sl] = v ? (uint32_t)fcx[lj] : 255u; cy[sl] = v ? (uint32_t)fcy[lj] : 255u;       // cell (255, 255): never inside a window
        const int g = v ? (int)gidx[lj] : 0;                                                 // (an empty slot must not index the descriptors with LDS garbage)
        d0[sl] = dB[2 * g]; d1[sl] = dB[2 * g + 1];
    }
    uint2 *rows = reinterpret_cast<uint2 *>(mat + (size_t)lane * NS + sl0);                  // a lane's share of row t: NS uint16_t at t * 64 * NS + lane * NS
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)                    // (interleaved by two the loop spills)
    for (int t = __builtin_amdgcn_readfirstlane(w); t < na0; t += 4) {                      // a wave per row
        const float x = qx[t], y = qy[t];
        const uint4 a0 = qd[2 * t], a1 = qd[2 * t + 1];
        int c0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)); if (c0 < 0) c0 = 0;   // Frame.cc:656-674
        int c1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)); if (c1 > SI_COLS - 1) c1 = SI_COLS - 1;
        int r0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)); if (r0 < 0) r0 = 0;
        int r1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)); if (r1 > SI_ROWS - 1) r1 = SI_ROWS - 1;
        const bool any = !(c0 >= SI_COLS || c1 < 0 || r0 >= SI_ROWS || r1 < 0);             // si_register_loop's early `continue`s: an empty row
        if (!any) c0 = 256;                                                                  // no cell reaches it: dcx wraps above cw
        const uint32_t cw = any ? (uint32_t)(c1 - c0) : 0u, rh = (uint32_t)(r1 - r0);
        uint32_t e[4];
#pragma unroll
        for (int sl = 0; sl < 4; sl++) {                                                     // branch-free
            const uint32_t dcx = cx[sl] - (uint32_t)c0, dcy = cy[sl] - (uint32_t)r0;
            const uint32_t dist = (uint32_t)hamming256(a0, a1, d0[sl], d1[sl]);
            const bool c = ((int)(dcx <= cw) & (int)(dcy <= rh) & (int)(fabsf(__fsub_rn(kx[sl], x)) < r) & (int)(fabsf(__fsub_rn(ky[sl], y)) < r)) != 0;
            e[sl] = c ? dist : 0xFFFFu;
        }
        rows[(size_t)t * (16 * NS)] = make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));  // (a row is 64 * NS * 2 bytes = 16 * NS uint2)
    }
}

__global__ __launch_bounds__(256, 4) void k_si_rows(const orbhip_keypoint *kpA_, const uint8_t *descA_, const int32_t *nA,
                                                 const orbhip_keypoint *kpB_, const uint8_t *descB_, const int32_t *nB,
                                                 int max_n, size_t kp_stride, float min_x, float min_y, float max_x, float max_y,
                                                 int window, int maxn, const float *prev_, int32_t *m12_, SiRows W)
{
    __shared__ __attribute__((aligned(16))) uint4 qd[SIR_CAP * 2];           // F1 subset: descriptors, window centres
    __shared__ float qx[SIR_CAP], qy[SIR_CAP], fx[SIR_CAP], fy[SIR_CAP];     // F2 subset: position, grid cell, frame index
    __shared__ uint32_t ckey[SIR_CAP];                                        // F2 subset: (cell x * SI_ROWS + cell y) << 9 | subset index
    __shared__ uint16_t fcx[SIR_CAP], fcy[SIR_CAP], gidx[SIR_CAP], aidx[SIR_CAP];
    __shared__ int wcnt[2][4];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n1 = nA[pair], n2 = nB[pair];
    if (n1 > maxn || n2 > maxn) {                                            // (k_search_init reports the capacity error)
        if (tid == 0) { W.redo[pair] = 1; W.n0[pair] = 0; W.na0[pair] = 0; }
        return;
    }
    const orbhip_keypoint *kpA = kpA_ + (size_t)pair * kp_stride, *kpB = kpB_ + (size_t)pair * kp_stride;
    const uint4 *dA = reinterpret_cast<const uint4 *>(descA_ + (size_t)pair * kp_stride * 32);
    const uint4 *dB = reinterpret_cast<const uint4 *>(descB_ + (size_t)pair * kp_stride * 32);
    const float *prev = prev_ + (size_t)pair * max_n * 2;
    int32_t *m12 = m12_ + (size_t)pair * max_n;
    const float inv_w = __fdiv_rn((float)SI_COLS, __fsub_rn(max_x, min_x));       // Frame.cc:334-335
    const float inv_h = __fdiv_rn((float)SI_ROWS, __fsub_rn(max_y, min_y));
    // ---- octave-0 subset of F2 that PosInGrid accepts, index order kept (= insertion order of the grid); four chunks of loads in flight
    int n0 = 0, trip = 0;
    for (int i0 = 0; i0 < n2; i0 += 1024) {
        float fxs[4], fys[4]; int ocs[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = min(i0 + 256 * u + tid, n2 - 1);
            fxs[u] = kpB[i].x; fys[u] = kpB[i].y; ocs[u] = kpB[i].octave;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (i0 + 256 * u >= n2) break;                                   // uniform
            const int i = i0 + 256 * u + tid;
            const int px = (int)roundf(__fmul_rn(__fsub_rn(fxs[u], min_x), inv_w));          // round(), Frame.cc:718-719
            const int py = (int)roundf(__fmul_rn(__fsub_rn(fys[u], min_y), inv_h));
            const bool in = i < n2 && ocs[u] == 0 && px >= 0 && px < SI_COLS && py >= 0 && py < SI_ROWS;
            const int li = si_rows_slot(in, lane, w, wcnt[trip++ & 1], n0);
            if (in && li < SIR_CAP) {
                fx[li] = fxs[u]; fy[li] = fys[u]; fcx[li] = (uint16_t)px; fcy[li] = (uint16_t)py; gidx[li] = (uint16_t)i;
                ckey[li] = ((uint32_t)(px * SI_ROWS + py) << 9) | (uint32_t)li;
            }
        }
    }
    // ---- octave-0 subset of F1 (ORBmatcher.cc:726-728)
    int na0 = 0;
    for (int i0 = 0; i0 < n1; i0 += 1024) {
        int ocs[4];
#pragma unroll
        for (int u = 0; u < 4; u++) ocs[u] = kpA[min(i0 + 256 * u + tid, n1 - 1)].octave;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (i0 + 256 * u >= n1) break;                                   // uniform
            const int i = i0 + 256 * u + tid;
            const bool in = i < n1 && ocs[u] == 0;
            const int li = si_rows_slot(in, lane, w, wcnt[trip++ & 1], na0);
            if (in && li < SIR_CAP) aidx[li] = (uint16_t)i;
            if (i < n1) m12[i] = -1;
        }
    }
    const bool over = n0 > SIR_CAP || na0 > SIR_CAP;
    if (tid == 0) { W.n0[pair] = n0; W.na0[pair] = na0; W.redo[pair] = over ? 1 : 0; }
    if (over) return;                                                        // (m12 was reset, prev is untouched: k_search_init starts over)
    __syncthreads();
    // ---- the chain's records, and the F1 subset's window centres and descriptors for the rows
    for (int j = tid; j < n0; j += 256) {                                    // ord[j]: the subset points with a smaller (cell x, cell y, subset index)
        const uint32_t mine = ckey[j];
        uint32_t ord = 0;
        for (int k = 0; k < n0; k++) ord += ckey[k] < mine;
        W.frec[(size_t)pair * SIR_CAP + j] = ord | ((uint32_t)gidx[j] << 16);
    }
    for (int t = tid; t < na0; t += 256) {
        const int i1 = aidx[t];
        W.aidx[(size_t)pair * SIR_CAP + t] = (uint16_t)i1;
        qx[t] = prev[2 * i1]; qy[t] = prev[2 * i1 + 1];
        qd[2 * t] = dA[2 * i1]; qd[2 * t + 1] = dA[2 * i1 + 1];
    }
    __syncthreads();
    uint16_t *mat = W.mat + (size_t)pair * W.cap * W.cols;
    const float r = (float)window;
    if (n0 <= 4 * 64) si_rows_fill<4>(0, lane, w, n0, na0, fx, fy, fcx, fcy, gidx, qx, qy, qd, dB, mat, min_x, min_y, inv_w, inv_h, r);
    else
        for (int sl0 = 0; sl0 < 8; sl0 += 4) si_rows_fill<8>(sl0, lane, w, n0, na0, fx, fy, fcx, fcy, gidx, qx, qy, qd, dB, mat, min_x, min_y, inv_w, inv_h, r);
}

// The chain of the rows form: si_register_loop with everything state-free taken out.  A lane holds, per slot, vMatchedDistance,
// vnMatches21, ord and the frame index of its F2 points -- no positions and no descriptors of either frame.  The loop makes no store to
// global memory: m12[i1] == i2 holds at the end exactly where F1 point i1 still owns F2 point i2 (a displaced owner's entry goes back to
// -1, ORBmatcher.cc:768-772, and k_si_rows reset every entry to -1), so m12 is written once, from vnMatches21, after the loop.  With loads
// only, and the same number of them on every path through an iteration, the row loads keep their lead (a conditional store in the loop
// had the compiler wait for every outstanding load at the joins).  The F1 frame indices come 64 at a time, one per lane.
template <int NS>
__device__ __forceinline__ int si_chain_loop(int lane, int na0, const uint32_t *frec, const uint16_t *aidx, const uint16_t *mat, uint16_t *bm,
                                             int32_t *m12, float nn_ratio)
{
    int nmatches = 0;
    uint32_t ford[NS]; int fgi[NS], fmd[NS], fm21[NS];
#pragma unroll
    for (int sl = 0; sl < NS; sl++) {
        const uint32_t rec = frec[sl * 64 + lane];                           // (beyond n0: never read through a key, the rows hold 0xFFFF there)
        ford[sl] = rec & 0xFFFFu; fgi[sl] = (int)(rec >> 16); fmd[sl] = INT_MAX; fm21[sl] = -1;
    }
    if (na0 <= 0) return 0;
    const SiRowShare<NS> *rows = reinterpret_cast<const SiRowShare<NS> *>(mat) + lane;
    SiRowShare<NS> ring[SIR_PF];
#pragma unroll
    for (int u = 0; u < SIR_PF - 1; u++) ring[u] = rows[(size_t)min(u, na0 - 1) * 64];
    int qi = aidx[min(lane, na0 - 1)];
    for (int tc = 0; tc < na0; tc += 64) {
        const int qn = aidx[min(tc + 64 + lane, na0 - 1)];                  // the next 64 frame indices, 64 points ahead
        const int nc = min(64, na0 - tc);
        for (int u0 = 0; u0 < nc; u0 += SIR_PF) {
#pragma unroll
            for (int u = 0; u < SIR_PF; u++) {
                const int tl = u0 + u;
                if (tl >= nc) break;                                        // uniform
                // the load goes into the slot of the point before this one, which is dead: into this point's own slot it would be copied
                // there at the end of the iteration, behind a wait for it
                ring[(u + SIR_PF - 1) % SIR_PF] = rows[(size_t)min(tc + tl + SIR_PF - 1, na0 - 1) * 64];
                const SiRowShare<NS> cur = ring[u];
                // per lane the smallest key and the runner-up key (0xFFFFFFFF where the point is no candidate or already matched at a
                // distance <= this one, ORBmatcher.cc:749)
                uint32_t lk1 = 0xFFFFFFFFu, lk2 = 0xFFFFFFFFu; int best_sl = 0;
#pragma unroll
                for (int sl = 0; sl < NS; sl++) {
                    const int d = (int)((sl & 1) ? cur.w[sl >> 1] >> 16 : cur.w[sl >> 1] & 0xFFFFu);
                    const bool c = d != 0xFFFF && !(fmd[sl] <= d);
                    const uint32_t key = c ? ((uint32_t)d << 23) | ford[sl] : 0xFFFFFFFFu;
                    lk2 = min(lk2, max(lk1, key));                          // the larger of (best so far, new) is a runner-up
                    best_sl = key < lk1 ? sl : best_sl;
                    lk1 = min(lk1, key);
                }
                uint32_t k1 = lk1, k2 = lk2;
                wave_min2_u32_dpp(k1, k2);                                  // keys are unique: the wave's two smallest
                const int d2 = k2 == 0xFFFFFFFFu ? INT_MAX : (int)(k2 >> 23);
                if (k1 == 0xFFFFFFFFu) continue;                            // no candidate, or none below its vMatchedDistance
                const int best = (int)(k1 >> 23);
                if (!(best <= TH_LOW && (float)best < __fmul_rn((float)d2, nn_ratio))) continue;   // ORBmatcher.cc:764-766
                const int i1 = __builtin_amdgcn_readlane(qi, tl);
                const unsigned long long owner = __ballot(lk1 == k1);      // keys are unique: exactly one lane
                const int ol = __builtin_amdgcn_readfirstlane(__ffsll((long long)owner) - 1);
                const int bsl = __builtin_amdgcn_readlane(best_sl, ol);
                int old = -1, best_idx = 0;
#pragma unroll
                for (int sl = 0; sl < NS; sl++)
                    if (bsl == sl) {                                        // uniform
                        old = __builtin_amdgcn_readlane(fm21[sl], ol); best_idx = __builtin_amdgcn_readlane(fgi[sl], ol);
                        if (lane == ol) { fm21[sl] = i1; fmd[sl] = best; }
                    }
                if (old >= 0) nmatches--;                                   // ORBmatcher.cc:768-772
                nmatches++;
                if (lane == 0) bm[i1] = (uint16_t)best_idx;                 // its rotation-histogram entry is made after the loop
            }
        }
        qi = qn;
    }
#pragma unroll
    for (int sl = 0; sl < NS; sl++)
        if (fm21[sl] >= 0) m12[fm21[sl]] = fgi[sl];                         // every owner is a different F1 point
    return nmatches;
}

__global__ __launch_bounds__(64) void k_si_chain(const orbhip_keypoint *kpA_, const int32_t *nA, const orbhip_keypoint *kpB_, size_t kp_stride, int max_n,
                                                 float nn_ratio, int check_ori, int maxn, SiRows W, float *prev_, int32_t *m12_, int32_t *nmatches_)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sic_lds[];
    uint16_t *bm = reinterpret_cast<uint16_t *>(sic_lds);                  // [maxn] F2 index an F1 keypoint was matched to (0xFFFF = never)
    int8_t *bin_of = reinterpret_cast<int8_t *>(bm + maxn);                 // [maxn]
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (W.redo[pair]) return;
    const int n1 = nA[pair], n0 = W.n0[pair], na0 = W.na0[pair];
    const orbhip_keypoint *kpA = kpA_ + (size_t)pair * kp_stride, *kpB = kpB_ + (size_t)pair * kp_stride;
    float *prev = prev_ + (size_t)pair * max_n * 2;
    int32_t *m12 = m12_ + (size_t)pair * max_n;                             // (k_si_rows reset it)
    const uint32_t *frec = W.frec + (size_t)pair * SIR_CAP;
    const uint16_t *aidx = W.aidx + (size_t)pair * SIR_CAP;
    const uint16_t *mat = W.mat + (size_t)pair * W.cap * W.cols;
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    for (int i = lane; i < n1; i += 64) { bin_of[i] = -1; bm[i] = 0xFFFFu; }
    __syncthreads();
    int nmatches;
    if (n0 <= 4 * 64) nmatches = si_chain_loop<4>(lane, na0, frec, aidx, mat, bm, m12, nn_ratio);
    else nmatches = si_chain_loop<8>(lane, na0, frec, aidx, mat, bm, m12, nn_ratio);
    nmatches = si_tail(lane, n1, kpA, kpB, bm, bin_of, hist, s_keep, m12, prev, nmatches, check_ori);
    if (lane == 0) nmatches_[pair] = nmatches;
}

extern "C" int orbhip_search_for_initialization_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kpA, const uint8_t *d_descA, const int32_t *d_nA,
        const orbhip_keypoint *d_kpB, const uint8_t *d_descB, const int32_t *d_nB,
        int pairs, int max_n, size_t frame_stride_kp, float min_x, float min_y, float max_x, float max_y,
        int window_size, float nn_ratio, int check_orientation,
        float *d_prev_matched, int32_t *d_matches12, int32_t *d_nmatches)
{
    if (!ctx || !d_kpA || !d_descA || !d_nA || !d_kpB || !d_descB || !d_nB || pairs <= 0 || max_n <= 0 ||
        !d_prev_matched || !d_matches12 || !d_nmatches || !(max_x > min_x) || !(max_y > min_y))
        return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    int32_t *d_status = orbhip_ctx_status_internal(ctx);    // frames over capacity set ORBHIP_E_CAPACITY
    // LDS is sized from the caller's row capacity: every keypoint of a frame may be octave 0
    const int maxn = max_n < SI_MAXN ? max_n : SI_MAXN, cap0 = max_n < SI_CAP0 ? max_n : SI_CAP0;
    const size_t lds = (size_t)cap0 * (4 * 4 + 7 * 2) + (size_t)maxn * 3;
    // Only octave-0 keypoints take part (~0.22 x nFeatures), but any keypoint MAY be one, so the full carve is 33 bytes per keypoint of
    // capacity: 36 KB per single-wave workgroup at 1100 -- four per CU, and no room beside another kernel's workgroups.  So the pairs are
    // first tried with LDS for ORBHIP_SI_SMALL_CAP0 (default 512) octave-0 points per frame; a pair with more is flagged on the device and
    // done by a second launch with the full carve, which returns at once for the others (0 switches the first launch off).
    const int small_env = getenv("ORBHIP_SI_SMALL_CAP0") ? atoi(getenv("ORBHIP_SI_SMALL_CAP0")) : 512;
    int cap0_small = small_env > 0 && small_env < cap0 ? (small_env + 7) & ~7 : 0;
    const size_t lds_small = (size_t)cap0_small * (4 * 4 + 7 * 2) + (size_t)maxn * 3;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_search_init), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    // Up to 16 pairs per call the replay form first (see k_si_replay), beyond that the rows form (k_si_rows + k_si_chain); pairs a form cannot
    // finish are flagged on the device and done by the sequential kernel, which returns at once for the others.  Measured (tools/si_sweep.py,
    // VGA / 1000 features, ~220 octave-0 points per frame; ms per call, replay / register loops (ORBHIP_SI_ROWS=0) / rows form):
    //      1 pair   0.109 / 0.233 / 0.110        64: 0.133 / 0.241 / 0.116       512: 0.243 / 0.263 / 0.146
    //      8        0.111 / 0.235 / 0.113       128: 0.149 / 0.243 / 0.119      1023: 0.363 / 0.309 / 0.188
    //     32        0.119 / 0.239 / 0.115       256: 0.179 / 0.244 / 0.133
    // -- the rows form is ahead from 32 pairs on and within 3 us of the replay form below (k_si_rows 27 us + k_si_chain 69 us at one pair,
    // 73 + 102 us at 1023).  ORBHIP_SI_PARALLEL_MAX_PAIRS moves the switch (0: the sequential path alone; tests run every form).
    const int par_max = getenv("ORBHIP_SI_PARALLEL_MAX_PAIRS") ? atoi(getenv("ORBHIP_SI_PARALLEL_MAX_PAIRS")) : 16;
    const int32_t *d_redo = nullptr;
    int32_t *d_redo2 = nullptr;
    {
        SiWork W;
        W.cap0 = ((max_n < SIL_CAP ? max_n : SIL_CAP) + 7) & ~7; W.chunks = (W.cap0 + 63) / 64;
        const size_t P = (size_t)pairs;
        const size_t o_rec = 0, o_desc = o_rec + align256(16 * P * W.cap0), o_aidx = o_desc + align256(32 * P * W.cap0), o_n0 = o_aidx + align256(2 * P * W.cap0),
                     o_na0 = o_n0 + align256(4 * P), o_lkey = o_na0 + align256(4 * P), o_lli = o_lkey + align256(4 * P * W.chunks * SIL_K * 64),
                     o_count = o_lli + align256(2 * P * W.chunks * SIL_K * 64), o_redo = o_count + align256(4 * P * W.cap0), total = o_redo + align256(4 * P);
        const bool replay = pairs <= par_max && total <= ((size_t)1 << 30);
        if (replay) cap0_small = 0;                                // behind the replay form the sequential kernel only sees the few pairs that one handed back: one launch
        // Beyond the replay form's range the rows form (k_si_rows + k_si_chain) takes the place of the register loops; the pairs it flags
        // (more than SIR_CAP octave-0 points, or over capacity) are done by the two k_search_init launches below, which return at once for the
        // others.  ORBHIP_SI_ROWS=0 (development) restores the launches of before exactly.  The matrix: cap rows x cols uint16_t per pair
        // (512 KB at VGA / 1000 features, of which na0 rows x 64 * NS columns are touched: ~110 KB per pair, ~115 MB per 1023-pair call);
        // a request above 1 GB (the replay form's limit) keeps the register loops.
        SiRows R;
        R.cap = max_n < SIR_CAP ? max_n : SIR_CAP; R.cols = R.cap <= 256 ? 256 : 512;
        const size_t r_mat = 0, r_aidx = r_mat + align256(2 * P * R.cap * R.cols), r_frec = r_aidx + align256(2 * P * SIR_CAP), r_n0 = r_frec + align256(4 * P * SIR_CAP),
                     r_na0 = r_n0 + align256(4 * P), r_redo = r_na0 + align256(4 * P), r_total = r_redo + align256(4 * P);
        const bool rows_on = !(getenv("ORBHIP_SI_ROWS") && atoi(getenv("ORBHIP_SI_ROWS")) == 0);
        const bool rows = !replay && rows_on && r_total <= ((size_t)1 << 30);
        if (rows) cap0_small = 0;                                  // as behind the replay form: one launch for the pairs handed back
        const size_t form_bytes = replay ? total : rows ? r_total : 0;
        uint8_t *wb = nullptr;
        if (form_bytes || cap0_small) {                            // (one request: the small launch's flags sit behind the form's work area)
            wb = (uint8_t *)orbhip_ctx_work_internal(ctx, form_bytes + (cap0_small ? align256(4 * P) : 0));
            if (!wb) return ORBHIP_E_HIP;
            if (cap0_small) d_redo2 = (int32_t *)(wb + form_bytes);
        }
        if (rows) {
            R.mat = (uint16_t *)(wb + r_mat); R.aidx = (uint16_t *)(wb + r_aidx); R.frec = (uint32_t *)(wb + r_frec); R.n0 = (int32_t *)(wb + r_n0);
            R.na0 = (int32_t *)(wb + r_na0); R.redo = (int32_t *)(wb + r_redo);
            const size_t chain_lds = (size_t)maxn * 3 + 16;
            if (orb_lds_optin(reinterpret_cast<const void *>(k_si_chain), orbhip_ctx_device_internal(ctx), chain_lds)) return ORBHIP_E_HIP;
            hipLaunchKernelGGL(k_si_rows, dim3(pairs), dim3(256), 0, st, d_kpA, d_descA, d_nA, d_kpB, d_descB, d_nB, max_n, frame_stride_kp, min_x, min_y,
                               max_x, max_y, window_size, maxn, d_prev_matched, d_matches12, R);
            hipLaunchKernelGGL(k_si_chain, dim3(pairs), dim3(64), chain_lds, st, d_kpA, d_nA, d_kpB, frame_stride_kp, max_n, nn_ratio, check_orientation,
                               maxn, R, d_prev_matched, d_matches12, d_nmatches);
            d_redo = R.redo;
            if (getenv("ORBHIP_SI_DEBUG")) {                       // development: how many pairs the rows form handed back
                std::vector<int32_t> h(pairs);
                if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(h.data(), R.redo, 4 * (size_t)pairs, hipMemcpyDeviceToHost) == hipSuccess) {
                    int nredo = 0;
                    for (int v : h) nredo += v != 0;
                    fprintf(stderr, "[orbhip] SearchForInitialization (rows form): %d of %d pairs fall back to the sequential kernel\n", nredo, pairs);
                }
            }
        }
        if (replay) {
            W.rec = (float4 *)(wb + o_rec); W.desc = (uint4 *)(wb + o_desc); W.aidx = (uint16_t *)(wb + o_aidx); W.n0 = (int32_t *)(wb + o_n0);
            W.na0 = (int32_t *)(wb + o_na0); W.lkey = (uint32_t *)(wb + o_lkey); W.lli = (uint16_t *)(wb + o_lli); W.count = (int32_t *)(wb + o_count);
            W.redo = (int32_t *)(wb + o_redo);
            const size_t prep_lds = (size_t)W.cap0 * 6 + 16, rep_lds = (size_t)W.cap0 * 12 + (size_t)SIL_K * 64 * 6 + (size_t)maxn * 3 + 16;
            if (orb_lds_optin(reinterpret_cast<const void *>(k_si_prep), orbhip_ctx_device_internal(ctx), prep_lds) ||
                orb_lds_optin(reinterpret_cast<const void *>(k_si_replay), orbhip_ctx_device_internal(ctx), rep_lds)) return ORBHIP_E_HIP;
            hipLaunchKernelGGL(k_si_prep, dim3(pairs), dim3(64), prep_lds, st, d_kpA, d_nA, d_kpB, d_descB, d_nB, frame_stride_kp, min_x, min_y, max_x, max_y, maxn, W);
            hipLaunchKernelGGL(k_si_candidates, dim3((W.cap0 + 3) / 4, pairs), dim3(256), 0, st, d_descA, frame_stride_kp, max_n, d_prev_matched, min_x, min_y,
                               max_x, max_y, window_size, W);
            hipLaunchKernelGGL(k_si_replay, dim3(pairs), dim3(64), rep_lds, st, d_kpA, d_nA, d_kpB, frame_stride_kp, max_n, nn_ratio, check_orientation, maxn, W,
                               d_prev_matched, d_matches12, d_nmatches);
            d_redo = W.redo;
            if (getenv("ORBHIP_SI_DEBUG")) {                       // development: how many pairs the replay form handed back
                std::vector<int32_t> h(pairs);
                if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(h.data(), W.redo, 4 * (size_t)pairs, hipMemcpyDeviceToHost) == hipSuccess) {
                    int nredo = 0;
                    for (int v : h) nredo += v != 0;
                    fprintf(stderr, "[orbhip] SearchForInitialization: %d of %d pairs fall back to the sequential kernel\n", nredo, pairs);
                }
            }
        }
    }
    if (cap0_small) {
        hipLaunchKernelGGL(k_search_init, dim3(pairs), dim3(64), lds_small, st, d_kpA, d_descA, d_nA,
                           d_kpB, d_descB, d_nB, max_n, frame_stride_kp, min_x, min_y, max_x, max_y, window_size, nn_ratio,
                           check_orientation, cap0_small, maxn, d_prev_matched, d_matches12, d_nmatches, d_status, d_redo, d_redo2);
        d_redo = d_redo2;
    }
    hipLaunchKernelGGL(k_search_init, dim3(pairs), dim3(64), lds, st, d_kpA, d_descA, d_nA,
                       d_kpB, d_descB, d_nB, max_n, frame_stride_kp, min_x, min_y, max_x, max_y, window_size, nn_ratio,
                       check_orientation, cap0, maxn, d_prev_matched, d_matches12, d_nmatches, d_status, d_redo, (int32_t *)nullptr);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

// vbPrevMatched initialisation (Tracking.cc:1497-1499: mvbPrevMatched[i] = mvKeysUn[i].pt), batched.
__global__ void k_prev_matched_init(const orbhip_keypoint *kp, size_t kp_stride, int frames, int max_n, float *xy)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= max_n || f >= frames) return;
    const orbhip_keypoint k = kp[(size_t)f * kp_stride + i];
    xy[((size_t)f * max_n + i) * 2] = k.x;
    xy[((size_t)f * max_n + i) * 2 + 1] = k.y;
}

extern "C" int orbhip_prev_matched_init_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp, size_t frame_stride_kp,
                                               int frames, int max_n, float *d_prev_matched)
{
    if (!ctx || !d_kp || !d_prev_matched || frames <= 0 || max_n <= 0) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(k_prev_matched_init, dim3((max_n + 255) / 256, frames), dim3(256), 0, orbhip_ctx_stream_internal(ctx),
                       d_kp, frame_stride_kp, frames, max_n, d_prev_matched);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}
