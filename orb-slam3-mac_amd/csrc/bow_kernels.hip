// bow_kernels.hip -- the bag-of-words side of the matchers: MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:327-403),
// the DBoW2 tree descent and BowVector / FeatureVector assembly (TemplatedVocabulary.h:1139-1260), and ORBmatcher::SearchByBoW for
// (KeyFrame, Frame) and (KeyFrame, KeyFrame) (src/ORBmatcher.cc:273-475, :827-967).
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "match_common.h"

// ---------------------------------------------------------------------------- distinctive descriptor
// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:327-403), batched over map points: one wave per point.
// The n x n distance matrix lives in LDS (u16); row i's median = sorted row [int(0.5*(n-1))] is found without
// sorting as the smallest v with #{j : D[i][j] <= v} >= k+1 (binary search over the 257 possible distances).
__global__ __launch_bounds__(64) void k_distinctive(const uint8_t *desc_, const int32_t *n_, int max_n, int32_t *best_idx, uint8_t *best_desc)
{
    extern __shared__ uint16_t dd[];               // [n][n]
    __shared__ uint32_t s_best;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = min(n_[p], max_n);
    const uint4 *D = reinterpret_cast<const uint4 *>(desc_ + (size_t)p * max_n * 32);
    if (lane == 0) s_best = 0xFFFFFFFFu;
    if (n <= 0) { if (lane == 0) best_idx[p] = 0; return; }
    for (int i = lane; i < n; i += 64) {
        const uint4 a0 = D[2 * i], a1 = D[2 * i + 1];
        for (int j = i + 1; j < n; j++) {                                   // MapPoint.cc:369-378
            const int d = hamming256(a0, a1, D[2 * j], D[2 * j + 1]);
            dd[i * n + j] = (uint16_t)d; dd[j * n + i] = (uint16_t)d;
        }
        dd[i * n + i] = 0;
    }
    __syncthreads();
    const int k = (int)(0.5 * (n - 1));                                     // MapPoint.cc:387
    for (int i = lane; i < n; i += 64) {
        int lo = 0, hi = 256;                                               // smallest v with count(<= v) >= k+1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int c = 0;
            for (int j = 0; j < n; j++) c += dd[i * n + j] <= mid;
            if (c >= k + 1) hi = mid; else lo = mid + 1;
        }
        atomicMin(&s_best, ((uint32_t)lo << 16) | (uint32_t)i);            // least median, first index on ties (:389-393)
    }
    __syncthreads();
    const int bi = (int)(s_best & 0xFFFFu);
    if (lane == 0) best_idx[p] = bi;
    if (best_desc && lane < 8) reinterpret_cast<uint32_t *>(best_desc + (size_t)p * 32)[lane] = reinterpret_cast<const uint32_t *>(D + 2 * bi)[lane];
}

extern "C" int orbhip_distinctive_descriptors_device(orbhip_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int points, int max_n,
                                                     int32_t *d_best_idx, uint8_t *d_best_desc)
{
    if (!ctx || !d_desc || !d_n || points <= 0 || max_n <= 0 || max_n > 256 || !d_best_idx) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    const size_t lds = sizeof(uint16_t) * (size_t)max_n * max_n;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_distinctive), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(k_distinctive, dim3(points), dim3(64), lds, orbhip_ctx_stream_internal(ctx), d_desc, d_n, max_n, d_best_idx, d_best_desc);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

// ---------------------------------------------------------------------------- BoW tree descent
// DBoW2 TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (TemplatedVocabulary.h:1218-1260),
// one thread per feature; the vocabulary is a flat CSR tree resident in HBM (node descriptors 32 B each).
__global__ __launch_bounds__(256) void k_bow_transform(const uint8_t *desc, const int32_t *n_, int frames, int max_n, size_t frame_stride,
                                                       const uint8_t *node_desc, const int32_t *child_start, const int32_t *child_ids,
                                                       const int32_t *node_word, const double *node_weight, int L, int levelsup,
                                                       int32_t *word_id, double *weight, int32_t *nid)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_[f] || i >= max_n) return;
    const uint4 *a = reinterpret_cast<const uint4 *>(desc + ((size_t)f * frame_stride + i) * 32);
    const uint4 a0 = a[0], a1 = a[1];
    const uint4 *nd = reinterpret_cast<const uint4 *>(node_desc);
    const int nid_level = L - levelsup;
    int out_nid = 0, final_id = 0, level = 0;
    int c0 = child_start[0], c1 = child_start[1];
    do {
        ++level;
        final_id = child_ids[c0];
        int best = hamming256(a0, a1, nd[2 * final_id], nd[2 * final_id + 1]);
        for (int c = c0 + 1; c < c1; c++) {
            const int id = child_ids[c];
            const int d = hamming256(a0, a1, nd[2 * id], nd[2 * id + 1]);
            if (d < best) { best = d; final_id = id; }
        }
        if (level == nid_level) out_nid = final_id;
        c0 = child_start[final_id]; c1 = child_start[final_id + 1];
    } while (c1 > c0);
    const size_t o = (size_t)f * max_n + i;
    word_id[o] = node_word[final_id]; weight[o] = node_weight[final_id]; nid[o] = out_nid;
}

extern "C" int orbhip_bow_transform_device(orbhip_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int frames, int max_n,
                                           size_t frame_stride, const uint8_t *d_node_desc, const int32_t *d_child_start,
                                           const int32_t *d_child_ids, const int32_t *d_node_word, const double *d_node_weight,
                                           int L, int levelsup, int32_t *d_word_id, double *d_weight, int32_t *d_nid)
{
    if (!ctx || !d_desc || !d_n || frames <= 0 || max_n <= 0 || !d_node_desc || !d_child_start || !d_child_ids || !d_node_word ||
        !d_node_weight || L <= 0 || !d_word_id || !d_weight || !d_nid) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(k_bow_transform, dim3((max_n + 255) / 256, frames), dim3(256), 0, orbhip_ctx_stream_internal(ctx), d_desc, d_n,
                       frames, max_n, frame_stride, d_node_desc, d_child_start, d_child_ids, d_node_word, d_node_weight, L, levelsup,
                       d_word_id, d_weight, d_nid);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

// ---------------------------------------------------------------------------- SearchByBoW (KeyFrame, Frame)
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:273-475, F.Nleft == -1).  A Frame feature belongs to exactly
// one vocabulary node, so the "already matched" rule (:321-322) only couples KF features of the SAME node: nodes are
// independent.  One wave per (keyframe, frame) pair, one lane per shared node (binary search of the frame's sorted node list),
// the node's KF features in order, the frame's descriptors and match slots LDS-resident.
struct BowSide { FeatVec fv; const orbhip_keypoint *kp; const uint8_t *desc; };
// KF_MODE: SearchByBoW(KeyFrame*, KeyFrame*) (ORBmatcher.cc:827-967): side F is the second keyframe with its own validity
// flags, the distance test is strict (:909) and the result is indexed by the first keyframe's feature (vpMatches12).
#define BOW_BIG_NODE 32        // frame features under one node from which the wave works on the node together
// BIG (round 4): frames / keyframes of more than 4096 features (to 16384) read the F side's descriptors from global memory
template <bool KF_MODE, bool BIG = false>
__global__ __launch_bounds__(64) void k_search_by_bow(BowSide K, const uint8_t *kf_valid_, const int32_t *nK_, BowSide F, const uint8_t *f_valid_,
                                                      const int32_t *nF_, int max_nodes, int max_n,
                                                      size_t kp_stride, float nn_ratio, int check_ori, int cap_n,
                                                      int32_t *match_f_, int32_t *nmatches_, int32_t *status, const int32_t *nleft_)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t bow_lds[];
    uint4 *dlds = reinterpret_cast<uint4 *>(bow_lds);                       // [cap_n][2] frame descriptors (BIG: absent)
    int16_t *mf = reinterpret_cast<int16_t *>(dlds + (BIG ? 0 : 2 * (size_t)cap_n));    // [cap_n] KF feature matched to frame feature j, -1 free, -2 invalid
    int16_t *inv = mf + cap_n;                                              // [cap_n] (KF_MODE) match of KF1 feature i
    int8_t *fbin = reinterpret_cast<int8_t *>(inv + (KF_MODE ? cap_n : 0)); // [cap_n] rotation bin of that match
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int nF = nF_[pair], nk = K.fv.nnodes[pair], nf = F.fv.nnodes[pair];
    int32_t *match_f = match_f_ + (size_t)pair * max_n;
    const int nK = KF_MODE ? nK_[pair] : 0;
    // rig frames (F.Nleft != -1, ORBmatcher.cc:338-359): frame features [0, nleft) are the left camera's, the rest the right camera's;
    // each keyframe feature keeps a best / second best per camera
    const int nleft = (!KF_MODE && nleft_) ? nleft_[pair] : -1;
    if (nF > cap_n || nF > max_n || nK > cap_n || nK > max_n || nk > max_nodes || nf > max_nodes) {
        if (lane == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; }
        return;
    }
    const uint8_t *fvalid = KF_MODE ? f_valid_ + (size_t)pair * max_n : nullptr;
    const int32_t *kids = K.fv.node_ids + (size_t)pair * max_nodes, *kst = K.fv.node_start + (size_t)pair * (max_nodes + 1), *kfe = K.fv.feat + (size_t)pair * max_n;
    const int32_t *fids = F.fv.node_ids + (size_t)pair * max_nodes, *fst = F.fv.node_start + (size_t)pair * (max_nodes + 1), *ffe = F.fv.feat + (size_t)pair * max_n;
    const uint8_t *kvalid = kf_valid_ + (size_t)pair * max_n;
    const orbhip_keypoint *kkp = K.kp + (size_t)pair * kp_stride, *fkp = F.kp + (size_t)pair * kp_stride;
    const uint4 *dK = reinterpret_cast<const uint4 *>(K.desc + (size_t)pair * kp_stride * 32);
    const uint4 *dF = reinterpret_cast<const uint4 *>(F.desc + (size_t)pair * kp_stride * 32);
    for (int i = lane; i < HISTO_LENGTH; i += 64) hist[i] = 0;
    for (int j = lane; j < nF; j += 64) {
        if (!BIG) { dlds[2 * j] = dF[2 * j]; dlds[2 * j + 1] = dF[2 * j + 1]; }
        fbin[j] = -1;
        mf[j] = (KF_MODE && !fvalid[j]) ? -2 : -1;                          // :887-891
    }
    if (KF_MODE) for (int i = lane; i < nK; i += 64) inv[i] = -1;
    __syncthreads();
    int mine = 0;
    for (int a0 = 0; a0 < nk; a0 += 64) {
        const int a = a0 + lane;
        if (a >= nk) continue;
        const int nid = kids[a];
        const int lo = node_lower_bound(fids, nf, nid);                      // the node in the frame's list (:435-442)
        if (lo >= nf || fids[lo] != nid) continue;
        const int f0 = fst[lo], f1 = fst[lo + 1];
        if (nleft < 0 && f1 - f0 >= BOW_BIG_NODE) continue;                 // big node: the whole wave works on it below
        for (int ik = kst[a]; ik < kst[a + 1]; ik++) {
            const int ri = kfe[ik];
            if (!kvalid[ri]) continue;                                       // :297-302
            const uint4 a0v = dK[2 * ri], a1v = dK[2 * ri + 1];
            int b1 = 256, b2 = 256, bi = -1, b1r = 256, b2r = 256, bir = -1;
            for (int jf = f0; jf < f1; jf++) {                               // :317-360
                const int rj = ffe[jf];
                if (mf[rj] != -1) continue;
                const int dist = (BIG ? hamming256(a0v, a1v, dF[2 * rj], dF[2 * rj + 1]) : hamming256(a0v, a1v, dlds[2 * rj], dlds[2 * rj + 1]));
                if (nleft < 0 || rj < nleft) {
                    if (dist < b1) { b2 = b1; b1 = dist; bi = rj; }
                    else if (dist < b2) b2 = dist;
                } else {
                    if (dist < b1r) { b2r = b1r; b1r = dist; bir = rj; }
                    else if (dist < b2r) b2r = dist;
                }
            }
            auto take = [&](int j) {
                mf[j] = (int16_t)ri;
                mine++;
                if (check_ori) {                                             // :376-388, :406-421
                    const int bin = rot_bin(kkp[ri].angle, fkp[j].angle);
                    atomicAdd(&hist[bin], 1); fbin[j] = (int8_t)bin;
                }
            };
            if (KF_MODE ? b1 < TH_LOW : b1 <= TH_LOW) {                // :362 / :909
                if ((float)b1 < __fmul_rn(nn_ratio, (float)b2)) take(bi);     // :364-391 / :911
                // the right camera's best: inside the left test's TH_LOW branch, no ratio test ("|| true", :393-396)
                if (nleft >= 0 && b1r <= TH_LOW) take(bir);
            }
        }
    }
    // ---- big nodes (coarse vocabularies, relocalisation with levelsup high: hundreds of features under one node): one node at a time, the
    // keyframe features in order (a frame feature claimed by an earlier one is skipped, :317-321), the 64 lanes over the node's frame
    // features; best = smallest (distance << 16 | position) -- the scan's strict "<" keeps the first of equal distances --, second best =
    // distance of the second smallest key.  Nodes are independent of each other (their frame features are disjoint), so doing these
    // after the lane-parallel pass changes nothing.
    if (nleft < 0) {
        for (int a = 0; a < nk; a++) {
            const int nid = kids[a];
            const int lo = node_lower_bound(fids, nf, nid);
            if (lo >= nf || fids[lo] != nid) continue;
            const int f0 = fst[lo], f1 = fst[lo + 1];
            if (f1 - f0 < BOW_BIG_NODE) continue;
            __syncthreads();
            // this lane's frame features of the node (positions lane, lane + 64, ...): indices kept in registers for the whole node
            int rjs[8];
#pragma unroll
            for (int u = 0; u < 8; u++) rjs[u] = f0 + lane + 64 * u < f1 ? ffe[f0 + lane + 64 * u] : -1;
            // the keyframe feature (index, validity, descriptor) is fetched two features ahead: the chain below would otherwise start with
            // two dependent global round trips per feature
            const int ik0 = kst[a], ik1 = kst[a + 1];
            int rq[2]; bool vq[2]; uint4 dq0[2], dq1[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                rq[u] = kfe[min(ik0 + u, ik1 - 1)]; vq[u] = kvalid[rq[u]] != 0; dq0[u] = dK[2 * rq[u]]; dq1[u] = dK[2 * rq[u] + 1];
            }
            for (int ik = ik0; ik < ik1; ik++) {
                const int ri = rq[0]; const bool vk = vq[0];
                const uint4 a0v = dq0[0], a1v = dq1[0];
                rq[0] = rq[1]; vq[0] = vq[1]; dq0[0] = dq0[1]; dq1[0] = dq1[1];
                rq[1] = kfe[min(ik + 2, ik1 - 1)]; vq[1] = kvalid[rq[1]] != 0; dq0[1] = dK[2 * rq[1]]; dq1[1] = dK[2 * rq[1] + 1];
                if (!vk) continue;
                uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (f0 + 64 * u >= f1) break;                           // uniform
                    const int rj = rjs[u];
                    if (rj < 0 || mf[rj] != -1) continue;
                    const uint32_t key = ((uint32_t)(BIG ? hamming256(a0v, a1v, dF[2 * rj], dF[2 * rj + 1]) : hamming256(a0v, a1v, dlds[2 * rj], dlds[2 * rj + 1])) << 16) | (uint32_t)(lane + 64 * u);
                    k2 = min(k2, max(k1, key)); k1 = min(k1, key);
                }
                for (int jf = f0 + 512 + lane; jf < f1; jf += 64) {           // (nodes of more than 512 frame features)
                    const int rj = ffe[jf];
                    if (mf[rj] != -1) continue;
                    const uint32_t key = ((uint32_t)(BIG ? hamming256(a0v, a1v, dF[2 * rj], dF[2 * rj + 1]) : hamming256(a0v, a1v, dlds[2 * rj], dlds[2 * rj + 1])) << 16) | (uint32_t)(jf - f0);
                    k2 = min(k2, max(k1, key)); k1 = min(k1, key);
                }
                wave_min2_u32_dpp(k1, k2);
                const int b1 = k1 == 0xFFFFFFFFu ? 256 : (int)(k1 >> 16), b2 = k2 == 0xFFFFFFFFu ? 256 : (int)(k2 >> 16);
                if ((KF_MODE ? b1 < TH_LOW : b1 <= TH_LOW) && (float)b1 < __fmul_rn(nn_ratio, (float)b2)) {
                    const int j = ffe[f0 + (int)(k1 & 0xFFFFu)];
                    if (lane == 0) {
                        mf[j] = (int16_t)ri;
                        mine++;
                        if (check_ori) {
                            const int bin = rot_bin(kkp[ri].angle, fkp[j].angle);
                            atomicAdd(&hist[bin], 1); fbin[j] = (int8_t)bin;
                        }
                    }
                    __syncthreads();                                         // mf[j] is read by every lane for the next keyframe feature
                }
            }
        }
    }
    mine = wave_sum_dpp(mine);
    __syncthreads();
    int removed = 0;
    if (check_ori) {                                                         // :445-470
        if (lane == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        for (int j = lane; j < nF; j += 64) {
            const int b = fbin[j];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            mf[j] = -1; removed++;
        }
        removed = wave_sum_dpp(removed);
    }
    __syncthreads();
    if (KF_MODE) {
        for (int j = lane; j < nF; j += 64) if (mf[j] >= 0) inv[mf[j]] = (int16_t)j;
        __syncthreads();
        for (int i = lane; i < nK; i += 64) match_f[i] = inv[i];
    } else {
        for (int j = lane; j < nF; j += 64) match_f[j] = mf[j];
    }
    if (lane == 0) nmatches_[pair] = mine - removed;
}

static int bow_launch(orbhip_ctx *ctx, bool kf_mode, const BowSide &K, const uint8_t *d_kf_valid, const int32_t *d_nK, const BowSide &F,
                      const uint8_t *d_f_valid, const int32_t *d_nF, int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio,
                      int check_orientation, int32_t *d_match, int32_t *d_nmatches, const int32_t *d_nleft = nullptr)
{
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    const bool big = max_n > 4096;                               // (the match slots are int16: 16384 features at most)
    const int lim = big ? 16384 : 4096;
    const int cap_n = ((max_n < lim ? max_n : lim) + 7) & ~7;
    const size_t lds = (size_t)cap_n * ((big ? 0 : 32) + 2 + 1 + (kf_mode ? 2 : 0)) + 16;
    {
        const void *fn = kf_mode ? (big ? reinterpret_cast<const void *>(k_search_by_bow<true, true>) : reinterpret_cast<const void *>(k_search_by_bow<true, false>))
                                 : (big ? reinterpret_cast<const void *>(k_search_by_bow<false, true>) : reinterpret_cast<const void *>(k_search_by_bow<false, false>));
        if (orb_lds_optin(fn, orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    }
#define BOW_LAUNCH(KF, BG, NL) hipLaunchKernelGGL((k_search_by_bow<KF, BG>), dim3(pairs), dim3(64), lds, orbhip_ctx_stream_internal(ctx), K, d_kf_valid, d_nK, F, d_f_valid, d_nF, \
                           max_nodes, max_n, frame_stride_kp, nn_ratio, check_orientation, cap_n, d_match, d_nmatches, orbhip_ctx_status_internal(ctx), NL)
    if (kf_mode) { if (big) BOW_LAUNCH(true, true, nullptr); else BOW_LAUNCH(true, false, nullptr); }
    else { if (big) BOW_LAUNCH(false, true, d_nleft); else BOW_LAUNCH(false, false, d_nleft); }
#undef BOW_LAUNCH
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

extern "C" int orbhip_search_by_bow_device(orbhip_ctx *ctx,
        const int32_t *d_kf_node_ids, const int32_t *d_kf_node_start, const int32_t *d_kf_feat, const int32_t *d_kf_nnodes,
        const uint8_t *d_kf_valid, const orbhip_keypoint *d_kf_kp, const uint8_t *d_kf_desc,
        const int32_t *d_f_node_ids, const int32_t *d_f_node_start, const int32_t *d_f_feat, const int32_t *d_f_nnodes,
        const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, const int32_t *d_nF,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_match_f, int32_t *d_nmatches)
{
    if (!ctx || !d_kf_node_ids || !d_kf_node_start || !d_kf_feat || !d_kf_nnodes || !d_kf_valid || !d_kf_kp || !d_kf_desc || !d_f_node_ids ||
        !d_f_node_start || !d_f_feat || !d_f_nnodes || !d_f_kp || !d_f_desc || !d_nF || pairs <= 0 || max_nodes <= 0 || max_n <= 0 ||
        !d_match_f || !d_nmatches) return ORBHIP_E_BADARG;
    BowSide K = {{d_kf_node_ids, d_kf_node_start, d_kf_feat, d_kf_nnodes}, d_kf_kp, d_kf_desc};
    BowSide F = {{d_f_node_ids, d_f_node_start, d_f_feat, d_f_nnodes}, d_f_kp, d_f_desc};
    return bow_launch(ctx, false, K, d_kf_valid, nullptr, F, nullptr, d_nF, pairs, max_nodes, max_n, frame_stride_kp, nn_ratio, check_orientation,
                      d_match_f, d_nmatches);
}

extern "C" int orbhip_search_by_bow_rig_device(orbhip_ctx *ctx,
        const int32_t *d_kf_node_ids, const int32_t *d_kf_node_start, const int32_t *d_kf_feat, const int32_t *d_kf_nnodes,
        const uint8_t *d_kf_valid, const orbhip_keypoint *d_kf_kp, const uint8_t *d_kf_desc,
        const int32_t *d_f_node_ids, const int32_t *d_f_node_start, const int32_t *d_f_feat, const int32_t *d_f_nnodes,
        const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, const int32_t *d_nF, const int32_t *d_nleft,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_match_f, int32_t *d_nmatches)
{
    if (!ctx || !d_kf_node_ids || !d_kf_node_start || !d_kf_feat || !d_kf_nnodes || !d_kf_valid || !d_kf_kp || !d_kf_desc || !d_f_node_ids ||
        !d_f_node_start || !d_f_feat || !d_f_nnodes || !d_f_kp || !d_f_desc || !d_nF || !d_nleft || pairs <= 0 || max_nodes <= 0 || max_n <= 0 ||
        !d_match_f || !d_nmatches) return ORBHIP_E_BADARG;
    BowSide K = {{d_kf_node_ids, d_kf_node_start, d_kf_feat, d_kf_nnodes}, d_kf_kp, d_kf_desc};
    BowSide F = {{d_f_node_ids, d_f_node_start, d_f_feat, d_f_nnodes}, d_f_kp, d_f_desc};
    return bow_launch(ctx, false, K, d_kf_valid, nullptr, F, nullptr, d_nF, pairs, max_nodes, max_n, frame_stride_kp, nn_ratio, check_orientation,
                      d_match_f, d_nmatches, d_nleft);
}

extern "C" int orbhip_search_by_bow_kf_device(orbhip_ctx *ctx,
        const int32_t *d_node_ids1, const int32_t *d_node_start1, const int32_t *d_feat1, const int32_t *d_nnodes1,
        const uint8_t *d_valid1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_valid2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const int32_t *d_n2,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches)
{
    if (!ctx || !d_node_ids1 || !d_node_start1 || !d_feat1 || !d_nnodes1 || !d_valid1 || !d_kp1 || !d_desc1 || !d_n1 || !d_node_ids2 ||
        !d_node_start2 || !d_feat2 || !d_nnodes2 || !d_valid2 || !d_kp2 || !d_desc2 || !d_n2 || pairs <= 0 || max_nodes <= 0 || max_n <= 0 ||
        !d_matches12 || !d_nmatches) return ORBHIP_E_BADARG;
    BowSide K = {{d_node_ids1, d_node_start1, d_feat1, d_nnodes1}, d_kp1, d_desc1};
    BowSide F = {{d_node_ids2, d_node_start2, d_feat2, d_nnodes2}, d_kp2, d_desc2};
    return bow_launch(ctx, true, K, d_valid1, d_n1, F, d_valid2, d_n2, pairs, max_nodes, max_n, frame_stride_kp, nn_ratio, check_orientation,
                      d_matches12, d_nmatches);
}

// ---------------------------------------------------------------------------- BowVector / FeatureVector assembly
// Second half of TemplatedVocabulary::transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1139-1208; TF_IDF weighting,
// L1 norm: the ORBvoc settings): from the per-feature (word, weight, node) of k_bow_transform build, per frame,
//   fv  = map<NodeId, vector<feature index>>  flattened as the CSR the SearchByBoW kernels read (nodes ascending, indices in feature order),
//   v   = map<WordId, sum of weights>          as sorted (word, value) arrays, L1-normalised.
// std::map order and accumulation order are reproduced exactly: keys (id << 16 | feature index) are sorted (bitonic, LDS), a word's
// weights are added in feature order (BowVector::addWeight), the norm is the SEQUENTIAL sum over ascending words (BowVector::normalize).
#define BV_THREADS 256
__device__ void bv_bitonic_sort(unsigned long long *k, int np2, int tid)
{
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (np2 >> 1); t += BV_THREADS) {
                const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == up) { k[lo] = b; k[hi] = a; }
            }
        }
    __syncthreads();
}
__global__ __launch_bounds__(BV_THREADS) void k_bow_vectors(const int32_t *wid_, const double *w_, const int32_t *nid_, const int32_t *n_, int max_n,
                                                            int cap_n, int max_nodes, int32_t *node_ids_, int32_t *node_start_, int32_t *feat_,
                                                            int32_t *nnodes_, int32_t *word_ids_, double *word_val_, int32_t *nwords_, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t bv_lds[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(bv_lds);      // [cap_n] (power of two)
    int32_t *head = reinterpret_cast<int32_t *>(keys + cap_n);                         // [cap_n] 1 where a new id starts / exclusive scan
    __shared__ int s_cnt, s_scan[BV_THREADS];
    __shared__ double s_norm;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = n_[f];
    const int32_t *wid = wid_ + (size_t)f * max_n, *nid = nid_ + (size_t)f * max_n;
    const double *w = w_ + (size_t)f * max_n;
    int32_t *node_ids = node_ids_ + (size_t)f * max_nodes, *node_start = node_start_ + (size_t)f * (max_nodes + 1), *feat = feat_ + (size_t)f * max_n;
    int32_t *word_ids = word_ids_ + (size_t)f * max_n;
    double *word_val = word_val_ + (size_t)f * max_n;
    if (n > cap_n || n > max_n) {
        if (tid == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nnodes_[f] = 0; nwords_[f] = 0; node_start[0] = 0; }
        return;
    }
    for (int pass = 0; pass < 2; pass++) {                   // pass 0: nodes -> FeatureVector, pass 1: words -> BowVector
        const int32_t *id = pass == 0 ? nid : wid;
        for (int i = tid; i < cap_n; i += BV_THREADS)        // stopped words (w <= 0) sort to the end and are dropped
            keys[i] = (i < n && w[i] > 0.0) ? (((unsigned long long)(uint32_t)id[i] << 16) | (unsigned)i) : ~0ull;
        if (tid == 0) s_cnt = 0;
        bv_bitonic_sort(keys, cap_n, tid);
        // number of kept entries and segment heads
        int mine = 0;
        for (int i = tid; i < cap_n; i += BV_THREADS) {
            const bool kept = keys[i] != ~0ull;
            mine += kept;
            head[i] = kept && (i == 0 || (keys[i] >> 16) != (keys[i - 1] >> 16)) ? 1 : 0;
        }
        atomicAdd(&s_cnt, mine);
        __syncthreads();
        const int m = s_cnt;
        // exclusive scan of head[] in blocks of cap_n / BV_THREADS consecutive entries per thread
        const int per = (cap_n + BV_THREADS - 1) / BV_THREADS, b0 = tid * per;
        int loc = 0;
        for (int i = b0; i < min(b0 + per, cap_n); i++) loc += head[i];
        s_scan[tid] = loc;
        __syncthreads();
        if (tid == 0) { int run = 0; for (int t = 0; t < BV_THREADS; t++) { const int v = s_scan[t]; s_scan[t] = run; run += v; } s_cnt = run; }
        __syncthreads();
        const int nseg = s_cnt;
        if (nseg > (pass == 0 ? max_nodes : max_n)) { if (tid == 0) atomicExch(status, ORBHIP_E_CAPACITY); }
        int run = s_scan[tid];
        for (int i = b0; i < min(b0 + per, cap_n); i++) {
            if (i >= m) break;
            const int seg = run + head[i] - 1;               // index of the segment entry i belongs to
            if (head[i]) {
                run++;
                if (pass == 0) { if (seg < max_nodes) { node_ids[seg] = (int32_t)(keys[i] >> 16); node_start[seg] = i; } }
                else if (seg < max_n) word_ids[seg] = (int32_t)(keys[i] >> 16);
            }
            if (pass == 0) feat[i] = (int32_t)(keys[i] & 0xFFFFu);
            else head[i] = head[i] ? -(seg + 1) : 0;         // mark heads with their segment for the sums below
        }
        __syncthreads();
        if (pass == 0) {
            if (tid == 0) { nnodes_[f] = min(nseg, max_nodes); node_start[min(nseg, max_nodes)] = m; }
        } else {
            // a word's weights in feature order (addWeight), one thread per word
            for (int i = tid; i < m; i += BV_THREADS) {
                if (head[i] >= 0) continue;
                const int seg = -head[i] - 1;
                double acc = 0.0;
                const unsigned long long wkey = keys[i] >> 16;
                for (int j = i; j < m && (keys[j] >> 16) == wkey; j++) acc += w[(int)(keys[j] & 0xFFFFu)];
                if (seg < max_n) word_val[seg] = acc;
            }
            __syncthreads();
            __threadfence_block();
            if (tid == 0) {                                   // BowVector::normalize(L1): sequential sum in ascending word order
                const int nw = min(nseg, max_n);
                double norm = 0.0;
                for (int k2 = 0; k2 < nw; k2++) norm += fabs(word_val[k2]);
                s_norm = norm;
                nwords_[f] = nw;
            }
            __syncthreads();
            if (s_norm > 0.0) {
                const double norm = s_norm;
                for (int k2 = tid; k2 < min(nseg, max_n); k2 += BV_THREADS) word_val[k2] /= norm;
            }
        }
        __syncthreads();
    }
}

extern "C" int orbhip_bow_vectors_device(orbhip_ctx *ctx, const int32_t *d_word_id, const double *d_weight, const int32_t *d_node_id,
                                         const int32_t *d_n, int frames, int max_n, int max_nodes,
                                         int32_t *d_node_ids, int32_t *d_node_start, int32_t *d_feat, int32_t *d_nnodes,
                                         int32_t *d_bow_word, double *d_bow_value, int32_t *d_nwords)
{
    if (!ctx || !d_word_id || !d_weight || !d_node_id || !d_n || frames <= 0 || max_n <= 0 || max_n > 4096 || max_nodes <= 0 || !d_node_ids ||
        !d_node_start || !d_feat || !d_nnodes || !d_bow_word || !d_bow_value || !d_nwords) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    int cap_n = 64;
    while (cap_n < max_n) cap_n <<= 1;
    const size_t lds = (size_t)cap_n * (8 + 4) + 16;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_bow_vectors), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(k_bow_vectors, dim3(frames), dim3(BV_THREADS), lds, orbhip_ctx_stream_internal(ctx), d_word_id, d_weight, d_node_id, d_n, max_n,
                       cap_n, max_nodes, d_node_ids, d_node_start, d_feat, d_nnodes, d_bow_word, d_bow_value, d_nwords, orbhip_ctx_status_internal(ctx));
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}
