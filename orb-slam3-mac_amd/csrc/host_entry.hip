// host_entry.hip -- host-pointer forms of the matcher / pose-optimisation entry points (include/orbhip.h): what an ORBmatcher or
// Optimizer method with the reference's signature needs for ONE frame.  No computation happens on the host.
//
// Round 4: a call used to issue 8-17 hipMemcpyAsync from PAGEABLE host vectors (each one staged and waited for by
// the runtime) and 2-4 copies back.  Now every call lays its arrays out in ONE blob -- inputs | in/outs | outputs | device-only buffers --
// that exists twice, in the context's device arena and in its page-locked host arena: the inputs are gathered into the host blob by
// memcpy and leave in ONE host-to-device copy, the kernels run on the device blob, in/outs + outputs come back in ONE device-to-host
// copy with the context's status word beside them, ONE synchronisation, and the results are scattered to the caller's arrays.
// The *_resident forms take the train side (keypoints + descriptors) as DEVICE pointers: the extractor's result arrays of the frame that
// was extracted a moment ago (orbhip_extractor_last_frame), so Tracking's matchers upload their queries only.
#include "orb_internal.h"
#include "ctx_internal.h"
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct HostCall {
    enum Kind { K_IN = 0, K_INOUT = 1, K_OUT = 2, K_BUF = 3 };
    struct Item { Kind k; const void *src; void *dst; size_t bytes, reserve, off; };
    orbhip_ctx *ctx; hipStream_t s;
    std::vector<Item> items;
    uint8_t *base, *host;                  // device blob, page-locked mirror
    size_t up_end, dl_start, dl_end, total;
    int32_t zero; int a_status; bool redirected;
    explicit HostCall(orbhip_ctx *c) : ctx(c), s(orbhip_ctx_stream_internal(c)), base(nullptr), host(nullptr), up_end(0), dl_start(0), dl_end(0), total(0), zero(0), a_status(-1), redirected(false) { items.reserve(32); }
    ~HostCall() { if (redirected) orbhip_ctx_redirect_status_internal(ctx, nullptr); }
    // `reserve` >= bytes: the array's size on the device (rows of a common stride); src == nullptr: an optional input that is absent
    int add(Kind k, const void *src, void *dst, size_t bytes, size_t reserve) { items.push_back({k, src, dst, bytes, reserve > bytes ? reserve : bytes, 0}); return (int)items.size() - 1; }
    int in(const void *src, size_t bytes, size_t reserve = 0) { return add(K_IN, src, nullptr, src ? bytes : 0, reserve); }
    int inout(void *p, size_t bytes, size_t reserve = 0) { return add(K_INOUT, p, p, bytes, reserve); }
    int out(void *dst, size_t bytes, size_t reserve = 0) { return add(K_OUT, nullptr, dst, bytes, reserve); }
    int buf(size_t bytes) { return add(K_BUF, nullptr, nullptr, 0, bytes); }
    int commit()
    {
        // the kernels' status word is an in/out slot of this call's blob: uploaded as 0 with the inputs, back with the outputs
        if (!pageable()) a_status = add(K_INOUT, &zero, nullptr, 4, 0);
        size_t off = 0;
        for (int k = K_IN; k <= K_BUF; k++) {
            if (k == K_INOUT) dl_start = off;
            for (Item &it : items) if (it.k == k) { it.off = off; off += align256(it.reserve ? it.reserve : 1); }
            if (k == K_INOUT) up_end = off;
            if (k == K_OUT) dl_end = off;
        }
        total = off;
        if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
        base = (uint8_t *)orbhip_ctx_scratch_internal(ctx, total + 256);
        host = (uint8_t *)orbhip_ctx_pinned_internal(ctx, dl_end + 256);         // + the status word behind the outputs
        if (!base || !host) return ORBHIP_E_HIP;
        if (pageable()) {                                                        // round 3's transfer pattern, kept for A/B measurements
            for (const Item &it : items)
                if (it.k <= K_INOUT && it.src && it.bytes && hipMemcpyAsync(base + it.off, it.src, it.bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
                    orbhip_set_last_error_internal("hipMemcpyAsync (host -> device staging)"); return ORBHIP_E_HIP;
                }
            return ORBHIP_OK;
        }
        for (const Item &it : items) if (it.k <= K_INOUT && it.src && it.bytes) memcpy(host + it.off, it.src, it.bytes);
        if (up_end && hipMemcpyAsync(base, host, up_end, hipMemcpyHostToDevice, s) != hipSuccess) { orbhip_set_last_error_internal("hipMemcpyAsync (host -> device blob)"); return ORBHIP_E_HIP; }
        orbhip_ctx_redirect_status_internal(ctx, ptr<int32_t>(a_status)); redirected = true;
        return ORBHIP_OK;
    }
    template <typename T> T *ptr(int i) const { return reinterpret_cast<T *>(base + items[i].off); }
    // one copy back, the status word beside it, one synchronisation; ORBHIP_E_CAPACITY etc. when a kernel flagged the frame
    // ORBHIP_HOST_PAGEABLE=1: one copy per array straight from / to the caller's pageable memory (what round 3 did)
    static bool pageable() { static const bool on = getenv("ORBHIP_HOST_PAGEABLE") && atoi(getenv("ORBHIP_HOST_PAGEABLE")) != 0; return on; }
    int finish()
    {
        int32_t *hst = reinterpret_cast<int32_t *>(host + dl_end);
        if (pageable()) {
            for (const Item &it : items)
                if ((it.k == K_INOUT || it.k == K_OUT) && it.dst && it.bytes) ORB_HIP_TRY(hipMemcpyAsync(it.dst, base + it.off, it.bytes, hipMemcpyDeviceToHost, s));
            ORB_HIP_TRY(hipStreamSynchronize(s));
            ORB_HIP_TRY(hipMemcpy(hst, orbhip_ctx_status_internal(ctx), sizeof(int32_t), hipMemcpyDeviceToHost));
            if (*hst) {
                const int st = *hst;
                ORB_HIP_TRY(hipMemset(orbhip_ctx_status_internal(ctx), 0, sizeof(int32_t)));
                orbhip_set_last_error_internal("device-side capacity exceeded in a matcher kernel");
                return st;
            }
            return ORBHIP_OK;
        }
        orbhip_ctx_redirect_status_internal(ctx, nullptr); redirected = false;
        ORB_HIP_TRY(hipMemcpyAsync(host + dl_start, base + dl_start, dl_end - dl_start, hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        hst = reinterpret_cast<int32_t *>(host + items[a_status].off);
        if (*hst) {
            orbhip_set_last_error_internal("device-side capacity exceeded in a matcher kernel");
            return *hst;
        }
        for (const Item &it : items) if ((it.k == K_INOUT || it.k == K_OUT) && it.dst && it.bytes) memcpy(it.dst, host + it.off, it.bytes);
        return ORBHIP_OK;
    }
};
}  // namespace

// train side: host arrays (kp / desc) or, when d_kp_res / d_desc_res are given, arrays already on the device
static int sbp_host(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                    const orbhip_keypoint *kp, const uint8_t *desc, const orbhip_keypoint *d_kp_res, const uint8_t *d_desc_res,
                    const float *u_right, int n, int nleft, const int32_t *mirror,
                    float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                    int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out)
{
    if (!ctx || nq < 0 || n < 0 || (nq && (!q || !desc_q)) || (n && ((!kp && !d_kp_res) || (!desc && !d_desc_res) || !train_match_inout)) || !nmatches_out ||
        (mode != 0 && mode != 1))
        return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    if (nq == 0 || n == 0) return ORBHIP_OK;
    HostCall H(ctx);
    const int a_q = H.in(q, sizeof(orbhip_proj_query) * (size_t)nq), a_dq = H.in(desc_q, 32 * (size_t)nq);
    const int a_kp = H.in(d_kp_res ? nullptr : kp, sizeof(orbhip_keypoint) * (size_t)n), a_d = H.in(d_desc_res ? nullptr : desc, 32 * (size_t)n);
    const int a_ur = H.in(u_right, 4 * (size_t)n), a_mi = H.in(nleft >= 0 ? mirror : nullptr, 4 * (size_t)n);
    const int a_nq = H.in(&nq, 4), a_n = H.in(&n, 4), a_nl = H.in(&nleft, 4);
    const int a_tm = H.inout(train_match_inout, 4 * (size_t)n), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const orbhip_keypoint *dkp = d_kp_res ? d_kp_res : H.ptr<orbhip_keypoint>(a_kp);
    const uint8_t *dd = d_desc_res ? d_desc_res : H.ptr<uint8_t>(a_d);
    const float *dur = u_right ? H.ptr<float>(a_ur) : nullptr;
    int rc;
    if (nleft >= 0)
        rc = orbhip_search_by_projection_rig_device(ctx, mode, H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq), H.ptr<int32_t>(a_nq), nq, dkp, dd, H.ptr<int32_t>(a_n),
                                                    H.ptr<int32_t>(a_nl), mirror ? H.ptr<int32_t>(a_mi) : nullptr, n, (size_t)n, 1, min_x, min_y, max_x, max_y, th_high,
                                                    nn_ratio, check_orientation, H.ptr<int32_t>(a_tm), H.ptr<int32_t>(a_nm));
    else if (mode == 0)
        rc = orbhip_search_by_projection_device(ctx, H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq), H.ptr<int32_t>(a_nq), nq, dkp, dd, dur, H.ptr<int32_t>(a_n), n,
                                                (size_t)n, 1, min_x, min_y, max_x, max_y, th_high, check_orientation, H.ptr<int32_t>(a_tm), H.ptr<int32_t>(a_nm));
    else
        rc = orbhip_search_local_map_device(ctx, H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq), H.ptr<int32_t>(a_nq), nq, dkp, dd, dur, H.ptr<int32_t>(a_n), n,
                                            (size_t)n, 1, min_x, min_y, max_x, max_y, th_high, nn_ratio, H.ptr<int32_t>(a_tm), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();                                   // ORBHIP_E_CAPACITY when the frame exceeds the kernel's limits
}

extern "C" int orbhip_search_by_projection_host(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                                const orbhip_keypoint *kp, const uint8_t *desc, const float *u_right, int n,
                                                float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                                int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out)
{
    return sbp_host(ctx, mode, q, desc_q, nq, kp, desc, nullptr, nullptr, u_right, n, -1, nullptr, min_x, min_y, max_x, max_y, th_high, nn_ratio, check_orientation,
                    train_match_inout, nmatches_out);
}

extern "C" int orbhip_search_by_projection_host_resident(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                                         const orbhip_keypoint *kp_host, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *u_right, int n,
                                                         float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                                         int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out)
{
    if (n && (!d_desc || (!d_kp && !kp_host))) return ORBHIP_E_BADARG;
    return sbp_host(ctx, mode, q, desc_q, nq, d_kp ? nullptr : kp_host, nullptr, d_kp, d_desc, u_right, n, -1, nullptr, min_x, min_y, max_x, max_y, th_high, nn_ratio, check_orientation,
                    train_match_inout, nmatches_out);
}

extern "C" int orbhip_search_by_projection_rig_host(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                                    const orbhip_keypoint *kp, const uint8_t *desc, int n, int nleft, const int32_t *mirror,
                                                    float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                                    int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out)
{
    if (nleft < 0 || nleft > n) return ORBHIP_E_BADARG;
    return sbp_host(ctx, mode, q, desc_q, nq, kp, desc, nullptr, nullptr, nullptr, n, nleft, mirror, min_x, min_y, max_x, max_y, th_high, nn_ratio, check_orientation,
                    train_match_inout, nmatches_out);
}

static int si_host(orbhip_ctx *ctx, const orbhip_keypoint *kpA, const uint8_t *descA, int nA, const orbhip_keypoint *kpB, const uint8_t *descB,
                   const orbhip_keypoint *d_kpB_res, const uint8_t *d_descB_res, int nB, float min_x, float min_y, float max_x, float max_y, int window_size,
                   float nn_ratio, int check_orientation, float *prev_matched_inout, int32_t *matches12_out, int32_t *nmatches_out)
{
    if (!ctx || nA < 0 || nB < 0 || (nA && (!kpA || !descA || !prev_matched_inout || !matches12_out)) || (nB && ((!kpB && !d_kpB_res) || (!descB && !d_descB_res))) ||
        !nmatches_out)
        return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    for (int i = 0; i < nA; i++) matches12_out[i] = -1;                 // vnMatches12 = vector<int>(F1.mvKeysUn.size(), -1), ORBmatcher.cc:713
    if (nA == 0 || nB == 0) return ORBHIP_OK;
    // the device entry point takes both sides at one row stride; a resident B side sits in the extractor's arrays, so both sides are
    // addressed as single rows there (batch 1: the stride is never used)
    const int mx = nA > nB ? nA : nB;
    HostCall H(ctx);
    const int a_ka = H.in(kpA, sizeof(orbhip_keypoint) * (size_t)nA, sizeof(orbhip_keypoint) * (size_t)mx), a_da = H.in(descA, 32 * (size_t)nA, 32 * (size_t)mx);
    const int a_kb = H.in(d_kpB_res ? nullptr : kpB, sizeof(orbhip_keypoint) * (size_t)nB, d_kpB_res ? 0 : sizeof(orbhip_keypoint) * (size_t)mx);      // (absent: 0 bytes)
    const int a_db = H.in(d_descB_res ? nullptr : descB, 32 * (size_t)nB, d_descB_res ? 0 : 32 * (size_t)mx);
    const int a_na = H.in(&nA, 4), a_nb = H.in(&nB, 4);
    const int a_pm = H.inout(prev_matched_inout, 8 * (size_t)nA, 8 * (size_t)mx), a_m = H.out(matches12_out, 4 * (size_t)nA, 4 * (size_t)mx), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_search_for_initialization_device(ctx, H.ptr<orbhip_keypoint>(a_ka), H.ptr<uint8_t>(a_da), H.ptr<int32_t>(a_na),
                                                           d_kpB_res ? d_kpB_res : H.ptr<orbhip_keypoint>(a_kb), d_descB_res ? d_descB_res : H.ptr<uint8_t>(a_db),
                                                           H.ptr<int32_t>(a_nb), 1, mx, (size_t)mx, min_x, min_y, max_x, max_y, window_size, nn_ratio, check_orientation,
                                                           H.ptr<float>(a_pm), H.ptr<int32_t>(a_m), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_search_for_initialization_host(orbhip_ctx *ctx, const orbhip_keypoint *kpA, const uint8_t *descA, int nA,
                                                     const orbhip_keypoint *kpB, const uint8_t *descB, int nB, float min_x, float min_y,
                                                     float max_x, float max_y, int window_size, float nn_ratio, int check_orientation,
                                                     float *prev_matched_inout, int32_t *matches12_out, int32_t *nmatches_out)
{
    return si_host(ctx, kpA, descA, nA, kpB, descB, nullptr, nullptr, nB, min_x, min_y, max_x, max_y, window_size, nn_ratio, check_orientation, prev_matched_inout,
                   matches12_out, nmatches_out);
}

extern "C" int orbhip_search_for_initialization_host_resident(orbhip_ctx *ctx, const orbhip_keypoint *kpA, const uint8_t *descA, int nA,
                                                              const orbhip_keypoint *kpB_host, const orbhip_keypoint *d_kpB, const uint8_t *d_descB, int nB, float min_x, float min_y,
                                                              float max_x, float max_y, int window_size, float nn_ratio, int check_orientation,
                                                              float *prev_matched_inout, int32_t *matches12_out, int32_t *nmatches_out)
{
    if (nB && (!d_descB || (!d_kpB && !kpB_host))) return ORBHIP_E_BADARG;
    return si_host(ctx, kpA, descA, nA, d_kpB ? nullptr : kpB_host, nullptr, d_kpB, d_descB, nB, min_x, min_y, max_x, max_y, window_size, nn_ratio, check_orientation, prev_matched_inout,
                   matches12_out, nmatches_out);
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) for ONE (keyframe, frame) pair from host memory: the two flattened
// FeatureVectors (node ids ascending, node_start [nnodes + 1], feature indices), the keyframe's "map point exists and is not bad"
// flags, keypoints (mvKeysUn / mvKeys, concatenated left | right for rig frames) and descriptors.  nleft < 0: F.Nleft == -1.
static int bow_host(orbhip_ctx *ctx,
        const int32_t *kf_node_ids, const int32_t *kf_node_start, const int32_t *kf_feat, int kf_nnodes, const uint8_t *kf_valid,
        const orbhip_keypoint *kf_kp, const uint8_t *kf_desc, int nK,
        const int32_t *f_node_ids, const int32_t *f_node_start, const int32_t *f_feat, int f_nnodes,
        const orbhip_keypoint *f_kp, const uint8_t *f_desc, const orbhip_keypoint *d_fkp_res, const uint8_t *d_fdesc_res, int nF, int nleft,
        float nn_ratio, int check_orientation, int32_t *match_f_out, int32_t *nmatches_out)
{
    if (!ctx || nK < 0 || nF < 0 || kf_nnodes < 0 || f_nnodes < 0 || !nmatches_out || (nF && !match_f_out) ||
        (kf_nnodes && (!kf_node_ids || !kf_node_start || !kf_feat || !kf_valid || !kf_kp || !kf_desc)) ||
        (f_nnodes && (!f_node_ids || !f_node_start || !f_feat || (!f_kp && !d_fkp_res) || (!f_desc && !d_fdesc_res))) || nleft > nF)
        return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    for (int i = 0; i < nF; i++) match_f_out[i] = -1;                   // vpMapPointMatches = vector<MapPoint*>(F.N, NULL), ORBmatcher.cc:277
    if (nK == 0 || nF == 0 || kf_nnodes == 0 || f_nnodes == 0) return ORBHIP_OK;
    const int mn = kf_nnodes > f_nnodes ? kf_nnodes : f_nnodes, mx = nK > nF ? nK : nF;
    HostCall H(ctx);
    const int a_ki = H.in(kf_node_ids, 4 * (size_t)kf_nnodes, 4 * (size_t)mn), a_ks = H.in(kf_node_start, 4 * (size_t)(kf_nnodes + 1), 4 * (size_t)(mn + 1));
    const int a_kf = H.in(kf_feat, 4 * (size_t)kf_node_start[kf_nnodes], 4 * (size_t)mx);
    const int a_fi = H.in(f_node_ids, 4 * (size_t)f_nnodes, 4 * (size_t)mn), a_fs = H.in(f_node_start, 4 * (size_t)(f_nnodes + 1), 4 * (size_t)(mn + 1));
    const int a_ff = H.in(f_feat, 4 * (size_t)f_node_start[f_nnodes], 4 * (size_t)mx);
    const int a_kk = H.in(kf_kp, sizeof(orbhip_keypoint) * (size_t)nK, sizeof(orbhip_keypoint) * (size_t)mx), a_kd = H.in(kf_desc, 32 * (size_t)nK, 32 * (size_t)mx);
    const int a_fk = H.in(d_fkp_res ? nullptr : f_kp, sizeof(orbhip_keypoint) * (size_t)nF, d_fkp_res ? 0 : sizeof(orbhip_keypoint) * (size_t)mx);
    const int a_fd = H.in(d_fdesc_res ? nullptr : f_desc, 32 * (size_t)nF, d_fdesc_res ? 0 : 32 * (size_t)mx);
    const int a_va = H.in(kf_valid, (size_t)nK, (size_t)mx);
    const int a_kn = H.in(&kf_nnodes, 4), a_fn = H.in(&f_nnodes, 4), a_nF = H.in(&nF, 4), a_nl = H.in(&nleft, 4);
    const int a_m = H.out(match_f_out, 4 * (size_t)nF, 4 * (size_t)mx), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const orbhip_keypoint *dfk = d_fkp_res ? d_fkp_res : H.ptr<orbhip_keypoint>(a_fk);
    const uint8_t *dfd = d_fdesc_res ? d_fdesc_res : H.ptr<uint8_t>(a_fd);
    int rc;
    if (nleft >= 0)
        rc = orbhip_search_by_bow_rig_device(ctx, H.ptr<int32_t>(a_ki), H.ptr<int32_t>(a_ks), H.ptr<int32_t>(a_kf), H.ptr<int32_t>(a_kn), H.ptr<uint8_t>(a_va),
                                             H.ptr<orbhip_keypoint>(a_kk), H.ptr<uint8_t>(a_kd), H.ptr<int32_t>(a_fi), H.ptr<int32_t>(a_fs), H.ptr<int32_t>(a_ff),
                                             H.ptr<int32_t>(a_fn), dfk, dfd, H.ptr<int32_t>(a_nF), H.ptr<int32_t>(a_nl), 1, mn, mx, (size_t)mx, nn_ratio,
                                             check_orientation, H.ptr<int32_t>(a_m), H.ptr<int32_t>(a_nm));
    else
        rc = orbhip_search_by_bow_device(ctx, H.ptr<int32_t>(a_ki), H.ptr<int32_t>(a_ks), H.ptr<int32_t>(a_kf), H.ptr<int32_t>(a_kn), H.ptr<uint8_t>(a_va),
                                         H.ptr<orbhip_keypoint>(a_kk), H.ptr<uint8_t>(a_kd), H.ptr<int32_t>(a_fi), H.ptr<int32_t>(a_fs), H.ptr<int32_t>(a_ff),
                                         H.ptr<int32_t>(a_fn), dfk, dfd, H.ptr<int32_t>(a_nF), 1, mn, mx, (size_t)mx, nn_ratio, check_orientation,
                                         H.ptr<int32_t>(a_m), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_search_by_bow_host(orbhip_ctx *ctx,
        const int32_t *kf_node_ids, const int32_t *kf_node_start, const int32_t *kf_feat, int kf_nnodes, const uint8_t *kf_valid,
        const orbhip_keypoint *kf_kp, const uint8_t *kf_desc, int nK,
        const int32_t *f_node_ids, const int32_t *f_node_start, const int32_t *f_feat, int f_nnodes,
        const orbhip_keypoint *f_kp, const uint8_t *f_desc, int nF, int nleft,
        float nn_ratio, int check_orientation, int32_t *match_f_out, int32_t *nmatches_out)
{
    return bow_host(ctx, kf_node_ids, kf_node_start, kf_feat, kf_nnodes, kf_valid, kf_kp, kf_desc, nK, f_node_ids, f_node_start, f_feat, f_nnodes, f_kp, f_desc,
                    nullptr, nullptr, nF, nleft, nn_ratio, check_orientation, match_f_out, nmatches_out);
}

extern "C" int orbhip_search_by_bow_host_resident(orbhip_ctx *ctx,
        const int32_t *kf_node_ids, const int32_t *kf_node_start, const int32_t *kf_feat, int kf_nnodes, const uint8_t *kf_valid,
        const orbhip_keypoint *kf_kp, const uint8_t *kf_desc, int nK,
        const int32_t *f_node_ids, const int32_t *f_node_start, const int32_t *f_feat, int f_nnodes,
        const orbhip_keypoint *f_kp_host, const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, int nF,
        float nn_ratio, int check_orientation, int32_t *match_f_out, int32_t *nmatches_out)
{
    if (f_nnodes && (!d_f_desc || (!d_f_kp && !f_kp_host))) return ORBHIP_E_BADARG;
    return bow_host(ctx, kf_node_ids, kf_node_start, kf_feat, kf_nnodes, kf_valid, kf_kp, kf_desc, nK, f_node_ids, f_node_start, f_feat, f_nnodes, d_f_kp ? nullptr : f_kp_host, nullptr,
                    d_f_kp, d_f_desc, nF, -1, nn_ratio, check_orientation, match_f_out, nmatches_out);
}

extern "C" int orbhip_search_for_triangulation_host(orbhip_ctx *ctx,
        const int32_t *nid1, const uint8_t *has_mp1, const orbhip_keypoint *kp1, const uint8_t *desc1, const float *u_right1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2,
        const uint8_t *has_mp2, const orbhip_keypoint *kp2, const uint8_t *desc2, const float *u_right2, int n2,
        const orbhip_tri_pair_general *pair, const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2,
        int nlevels, int check_orientation, int32_t *matches12_out, int32_t *nmatches_out)
{
    if (!ctx || n1 < 0 || n2 < 0 || nnodes2 < 0 || !pair || !nmatches_out || (n1 && (!nid1 || !has_mp1 || !kp1 || !desc1 || !matches12_out)) ||
        (n2 && (!has_mp2 || !kp2 || !desc2)) || (nnodes2 && (!node_ids2 || !node_start2 || !feat2)) || !level_sigma2_1 || !scale_factors2 || !level_sigma2_2)
        return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    for (int i = 0; i < n1; i++) matches12_out[i] = -1;                 // vMatches12 = vector<int>(pKF1->N, -1), ORBmatcher.cc:1017
    if (n1 == 0 || n2 == 0 || nnodes2 == 0) return ORBHIP_OK;
    const int mx = n1 > n2 ? n1 : n2;
    HostCall H(ctx);
    const int a_nid = H.in(nid1, 4 * (size_t)n1), a_mp1 = H.in(has_mp1, n1), a_ur1 = H.in(u_right1, 4 * (size_t)n1);
    const int a_ids = H.in(node_ids2, 4 * (size_t)nnodes2), a_st = H.in(node_start2, 4 * (size_t)(nnodes2 + 1)), a_fe = H.in(feat2, 4 * (size_t)node_start2[nnodes2]);
    const int a_mp2 = H.in(has_mp2, n2), a_ur2 = H.in(u_right2, 4 * (size_t)n2);
    const int a_kp1 = H.in(kp1, sizeof(orbhip_keypoint) * (size_t)n1, sizeof(orbhip_keypoint) * (size_t)mx);      // rows of mx entries: one stride for both sides
    const int a_kp2 = H.in(kp2, sizeof(orbhip_keypoint) * (size_t)n2, sizeof(orbhip_keypoint) * (size_t)mx);
    const int a_d1 = H.in(desc1, 32 * (size_t)n1, 32 * (size_t)mx), a_d2 = H.in(desc2, 32 * (size_t)n2, 32 * (size_t)mx);
    const int a_pair = H.in(pair, sizeof(*pair)), a_n1 = H.in(&n1, 4), a_n2 = H.in(&n2, 4), a_nn = H.in(&nnodes2, 4);
    const int a_m = H.out(matches12_out, 4 * (size_t)n1, 4 * (size_t)mx), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_search_for_triangulation_general_device(ctx, H.ptr<int32_t>(a_nid), H.ptr<uint8_t>(a_mp1), H.ptr<orbhip_keypoint>(a_kp1),
        H.ptr<uint8_t>(a_d1), u_right1 ? H.ptr<float>(a_ur1) : nullptr, H.ptr<int32_t>(a_n1), H.ptr<int32_t>(a_ids), H.ptr<int32_t>(a_st), H.ptr<int32_t>(a_fe),
        H.ptr<int32_t>(a_nn), H.ptr<uint8_t>(a_mp2), H.ptr<orbhip_keypoint>(a_kp2), H.ptr<uint8_t>(a_d2), u_right2 ? H.ptr<float>(a_ur2) : nullptr,
        H.ptr<int32_t>(a_n2), H.ptr<orbhip_tri_pair_general>(a_pair), 1, nnodes2, mx, (size_t)mx, level_sigma2_1, scale_factors2, level_sigma2_2, nlevels,
        check_orientation, H.ptr<int32_t>(a_m), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_match_and_triangulate_host(orbhip_ctx *ctx,
        const int32_t *nid1, const uint8_t *has_mp1, const orbhip_keypoint *kp1, const uint8_t *desc1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2,
        const uint8_t *has_mp2, const orbhip_keypoint *kp2, const uint8_t *desc2, int n2,
        const orbhip_tri_pair_general *pair, const orbhip_tri_pair_poses *poses, const float *level_sigma2_1, const float *level_sigma2_2,
        int nlevels, int check_orientation, int32_t *matches12_out, float *points12_out, int32_t *nmatches_out)
{
    if (!ctx || n1 < 0 || n2 < 0 || nnodes2 < 0 || !pair || !poses || !nmatches_out || (n1 && (!nid1 || !has_mp1 || !kp1 || !desc1 || !matches12_out || !points12_out)) ||
        (n2 && (!has_mp2 || !kp2 || !desc2)) || (nnodes2 && (!node_ids2 || !node_start2 || !feat2)) || !level_sigma2_1 || !level_sigma2_2)
        return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    for (int i = 0; i < n1; i++) { matches12_out[i] = -1; points12_out[3 * i] = points12_out[3 * i + 1] = points12_out[3 * i + 2] = 0.f; }
    if (n1 == 0 || n2 == 0 || nnodes2 == 0) return ORBHIP_OK;
    const int mx = n1 > n2 ? n1 : n2;
    HostCall H(ctx);
    const int a_nid = H.in(nid1, 4 * (size_t)n1), a_mp1 = H.in(has_mp1, n1);
    const int a_ids = H.in(node_ids2, 4 * (size_t)nnodes2), a_st = H.in(node_start2, 4 * (size_t)(nnodes2 + 1)), a_fe = H.in(feat2, 4 * (size_t)node_start2[nnodes2]);
    const int a_mp2 = H.in(has_mp2, n2);
    const int a_kp1 = H.in(kp1, sizeof(orbhip_keypoint) * (size_t)n1, sizeof(orbhip_keypoint) * (size_t)mx);
    const int a_kp2 = H.in(kp2, sizeof(orbhip_keypoint) * (size_t)n2, sizeof(orbhip_keypoint) * (size_t)mx);
    const int a_d1 = H.in(desc1, 32 * (size_t)n1, 32 * (size_t)mx), a_d2 = H.in(desc2, 32 * (size_t)n2, 32 * (size_t)mx);
    const int a_pair = H.in(pair, sizeof(*pair)), a_poses = H.in(poses, sizeof(*poses)), a_n1 = H.in(&n1, 4), a_n2 = H.in(&n2, 4), a_nn = H.in(&nnodes2, 4);
    const int a_m = H.out(matches12_out, 4 * (size_t)n1, 4 * (size_t)mx), a_pt = H.out(points12_out, 12 * (size_t)n1, 12 * (size_t)mx), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_match_and_triangulate_device(ctx, H.ptr<int32_t>(a_nid), H.ptr<uint8_t>(a_mp1), H.ptr<orbhip_keypoint>(a_kp1), H.ptr<uint8_t>(a_d1),
        H.ptr<int32_t>(a_n1), H.ptr<int32_t>(a_ids), H.ptr<int32_t>(a_st), H.ptr<int32_t>(a_fe), H.ptr<int32_t>(a_nn), H.ptr<uint8_t>(a_mp2),
        H.ptr<orbhip_keypoint>(a_kp2), H.ptr<uint8_t>(a_d2), H.ptr<int32_t>(a_n2), H.ptr<orbhip_tri_pair_general>(a_pair), H.ptr<orbhip_tri_pair_poses>(a_poses), 1,
        nnodes2, mx, (size_t)mx, level_sigma2_1, level_sigma2_2, nlevels, check_orientation, H.ptr<int32_t>(a_m), H.ptr<float>(a_pt), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();
}

// LocalMapping::CreateNewMapPoints' neighbour loop for one current keyframe: search -> create (flags updated) per neighbour, in order, on
// one blob.  Neighbours without keypoints or vocabulary nodes match nothing (their rows keep the reset values) and launch nothing.
extern "C" int orbhip_create_new_map_points_host(orbhip_ctx *ctx, const orbhip_newpoints_keyframe *cur, const orbhip_newpoints_keyframe *neigh,
        const orbhip_tri_pair_general *geom, const orbhip_newpoints_pair *pair, int n_neigh, int nlevels, int check_orientation,
        int32_t *matches12_out, float *x3D_out, uint8_t *outcome_out, int32_t *n_created_out, uint8_t *has_mp1_out)
{
    if (!ctx || !cur || n_neigh < 0 || (n_neigh && (!neigh || !geom || !pair || !n_created_out)) || cur->n < 0 ||
        (cur->n && (!cur->kp || !cur->desc || !cur->has_mp || !cur->nid || !matches12_out || !x3D_out || !outcome_out)) ||
        (cur->n && n_neigh && (!cur->level_sigma2 || !cur->scale_factors)) || (cur->u_right != nullptr) != (cur->depth != nullptr)) {
        orbhip_set_last_error_internal("orbhip_create_new_map_points_host: a required pointer of the current keyframe or of the outputs is NULL");
        return ORBHIP_E_BADARG;
    }
    const int n1 = cur->n;
    int mx = n1;
    for (int k = 0; k < n_neigh; k++) {
        const orbhip_newpoints_keyframe &f = neigh[k];
        if (f.n < 0 || f.nnodes < 0 || (f.n && (!f.kp || !f.desc || !f.has_mp)) || (f.nnodes && (!f.node_ids || !f.node_start || !f.feat)) ||
            !f.level_sigma2 || !f.scale_factors || (f.u_right != nullptr) != (f.depth != nullptr)) {
            orbhip_set_last_error_internal("orbhip_create_new_map_points_host: a required pointer of a neighbour keyframe is NULL");
            return ORBHIP_E_BADARG;
        }
        if (f.n > mx) mx = f.n;
    }
    for (int k = 0; k < n_neigh; k++) {
        n_created_out[k] = 0;
        for (size_t i = 0; i < (size_t)n1; i++) matches12_out[(size_t)k * n1 + i] = -1;
        memset(x3D_out + (size_t)k * n1 * 3, 0, 12 * (size_t)n1); memset(outcome_out + (size_t)k * n1, 0, (size_t)n1);
    }
    if (has_mp1_out && n1) memcpy(has_mp1_out, cur->has_mp, (size_t)n1);
    if (n1 == 0 || n_neigh == 0) return ORBHIP_OK;
    if (int rc = orbhip_newpoints_check_internal(pair, n_neigh, mx, nlevels)) return rc;
    HostCall H(ctx);
    const size_t kpb = sizeof(orbhip_keypoint);
    const int a_nid = H.in(cur->nid, 4 * (size_t)n1), a_ur1 = H.in(cur->u_right, 4 * (size_t)n1, 4 * (size_t)mx), a_dp1 = H.in(cur->depth, 4 * (size_t)n1, 4 * (size_t)mx);
    const int a_kp1 = H.in(cur->kp, kpb * n1, kpb * mx), a_raw1 = H.in(cur->kp_raw, kpb * n1, kpb * mx), a_d1 = H.in(cur->desc, 32 * (size_t)n1, 32 * (size_t)mx);
    const int a_n1 = H.in(&n1, 4);
    const int a_mp1 = has_mp1_out ? H.inout(has_mp1_out, n1, mx) : H.in(cur->has_mp, n1, mx);
    const int a_pair = H.in(pair, sizeof(*pair) * (size_t)n_neigh), a_geom = H.in(geom, sizeof(*geom) * (size_t)n_neigh);
    struct Slot { int ids, st, fe, mp2, ur2, dp2, kp2, raw2, d2, n2, nn, m, x, o, nc, nm; bool run; };
    std::vector<Slot> S(n_neigh);
    for (int k = 0; k < n_neigh; k++) {
        const orbhip_newpoints_keyframe &f = neigh[k];
        Slot &s = S[k];
        s.run = f.n > 0 && f.nnodes > 0;
        if (!s.run) continue;
        s.ids = H.in(f.node_ids, 4 * (size_t)f.nnodes); s.st = H.in(f.node_start, 4 * (size_t)(f.nnodes + 1)); s.fe = H.in(f.feat, 4 * (size_t)f.node_start[f.nnodes], 4 * (size_t)mx);
        s.mp2 = H.in(f.has_mp, f.n, mx); s.ur2 = H.in(f.u_right, 4 * (size_t)f.n, 4 * (size_t)mx); s.dp2 = H.in(f.depth, 4 * (size_t)f.n, 4 * (size_t)mx);
        s.kp2 = H.in(f.kp, kpb * f.n, kpb * mx); s.raw2 = H.in(f.kp_raw, kpb * f.n, kpb * mx); s.d2 = H.in(f.desc, 32 * (size_t)f.n, 32 * (size_t)mx);
        s.n2 = H.in(&f.n, 4); s.nn = H.in(&f.nnodes, 4);
        s.m = H.out(matches12_out + (size_t)k * n1, 4 * (size_t)n1, 4 * (size_t)mx); s.x = H.out(x3D_out + (size_t)k * n1 * 3, 12 * (size_t)n1, 12 * (size_t)mx);
        s.o = H.out(outcome_out + (size_t)k * n1, n1, mx); s.nc = H.out(n_created_out + k, 4); s.nm = H.buf(4);
    }
    if (int rc = H.commit()) return rc;
    for (int k = 0; k < n_neigh; k++) {
        const orbhip_newpoints_keyframe &f = neigh[k];
        const Slot &s = S[k];
        if (!s.run) continue;
        if (f.node_start[f.nnodes] > mx) { orbhip_set_last_error_internal("orbhip_create_new_map_points_host: a FeatureVector lists more features than the keyframe has"); return ORBHIP_E_BADARG; }
        int rc = orbhip_search_for_triangulation_general_device(ctx, H.ptr<int32_t>(a_nid), H.ptr<uint8_t>(a_mp1), H.ptr<orbhip_keypoint>(a_kp1), H.ptr<uint8_t>(a_d1),
            cur->u_right ? H.ptr<float>(a_ur1) : nullptr, H.ptr<int32_t>(a_n1), H.ptr<int32_t>(s.ids), H.ptr<int32_t>(s.st), H.ptr<int32_t>(s.fe), H.ptr<int32_t>(s.nn),
            H.ptr<uint8_t>(s.mp2), H.ptr<orbhip_keypoint>(s.kp2), H.ptr<uint8_t>(s.d2), f.u_right ? H.ptr<float>(s.ur2) : nullptr, H.ptr<int32_t>(s.n2),
            H.ptr<orbhip_tri_pair_general>(a_geom) + k, 1, f.nnodes, mx, (size_t)mx, cur->level_sigma2, f.scale_factors, f.level_sigma2, nlevels, check_orientation,
            H.ptr<int32_t>(s.m), H.ptr<int32_t>(s.nm));
        if (rc) return rc;
        rc = orbhip_newpoints_launch_internal(ctx, H.ptr<orbhip_keypoint>(a_kp1), cur->kp_raw ? H.ptr<orbhip_keypoint>(a_raw1) : nullptr,
            cur->u_right ? H.ptr<float>(a_ur1) : nullptr, cur->depth ? H.ptr<float>(a_dp1) : nullptr, H.ptr<int32_t>(a_n1),
            H.ptr<orbhip_keypoint>(s.kp2), f.kp_raw ? H.ptr<orbhip_keypoint>(s.raw2) : nullptr, f.u_right ? H.ptr<float>(s.ur2) : nullptr,
            f.depth ? H.ptr<float>(s.dp2) : nullptr, H.ptr<int32_t>(s.n2), H.ptr<int32_t>(s.m), H.ptr<orbhip_newpoints_pair>(a_pair) + k, 1, mx, (size_t)mx,
            cur->level_sigma2, cur->scale_factors, f.level_sigma2, f.scale_factors, nlevels, H.ptr<uint8_t>(a_mp1), H.ptr<uint8_t>(s.mp2),
            H.ptr<float>(s.x), H.ptr<uint8_t>(s.o), H.ptr<int32_t>(s.nc));
        if (rc) return rc;
    }
    return H.finish();
}

extern "C" int orbhip_fuse_search_host(orbhip_ctx *ctx, const orbhip_proj_query *q, const uint8_t *desc_q, int nq, const orbhip_keypoint *kp,
                                       const uint8_t *desc, const float *u_right, int n, const float *inv_level_sigma2, int nlevels,
                                       float min_x, float min_y, float max_x, float max_y, int32_t *best_idx_out, int32_t *best_dist_out)
{
    if (!ctx || nq < 0 || n < 0 || (nq && (!q || !desc_q || !best_idx_out || !best_dist_out)) || (n && (!kp || !desc)) || !inv_level_sigma2 || nlevels <= 0)
        return ORBHIP_E_BADARG;
    for (int i = 0; i < nq; i++) { best_idx_out[i] = -1; best_dist_out[i] = 256; }
    if (nq == 0 || n == 0) return ORBHIP_OK;
    HostCall H(ctx);
    const int a_q = H.in(q, sizeof(orbhip_proj_query) * (size_t)nq), a_dq = H.in(desc_q, 32 * (size_t)nq), a_kp = H.in(kp, sizeof(orbhip_keypoint) * (size_t)n);
    const int a_d = H.in(desc, 32 * (size_t)n), a_ur = H.in(u_right, 4 * (size_t)n), a_nq = H.in(&nq, 4), a_n = H.in(&n, 4);
    const int a_bi = H.out(best_idx_out, 4 * (size_t)nq), a_bd = H.out(best_dist_out, 4 * (size_t)nq);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_fuse_search_device(ctx, H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq), H.ptr<int32_t>(a_nq), nq, H.ptr<orbhip_keypoint>(a_kp),
                                             H.ptr<uint8_t>(a_d), u_right ? H.ptr<float>(a_ur) : nullptr, H.ptr<int32_t>(a_n), n, (size_t)n, 1, inv_level_sigma2,
                                             nlevels, min_x, min_y, max_x, max_y, H.ptr<int32_t>(a_bi), H.ptr<int32_t>(a_bd));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_search_by_bow_kf_host(orbhip_ctx *ctx,
        const int32_t *node_ids1, const int32_t *node_start1, const int32_t *feat1, int nnodes1, const uint8_t *valid1,
        const orbhip_keypoint *kp1, const uint8_t *desc1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2, const uint8_t *valid2,
        const orbhip_keypoint *kp2, const uint8_t *desc2, int n2,
        float nn_ratio, int check_orientation, int32_t *matches12_out, int32_t *nmatches_out)
{
    if (!ctx || n1 < 0 || n2 < 0 || nnodes1 < 0 || nnodes2 < 0 || !nmatches_out || (n1 && !matches12_out) ||
        (nnodes1 && (!node_ids1 || !node_start1 || !feat1 || !valid1 || !kp1 || !desc1)) ||
        (nnodes2 && (!node_ids2 || !node_start2 || !feat2 || !valid2 || !kp2 || !desc2))) return ORBHIP_E_BADARG;
    *nmatches_out = 0;
    for (int i = 0; i < n1; i++) matches12_out[i] = -1;                 // vpMatches12 = vector<MapPoint*>(vpMapPoints1.size(), NULL), ORBmatcher.cc:839
    if (n1 == 0 || n2 == 0 || nnodes1 == 0 || nnodes2 == 0) return ORBHIP_OK;
    const int mn = nnodes1 > nnodes2 ? nnodes1 : nnodes2, mx = n1 > n2 ? n1 : n2;
    HostCall H(ctx);
    const int a_i1 = H.in(node_ids1, 4 * (size_t)nnodes1, 4 * (size_t)mn), a_s1 = H.in(node_start1, 4 * (size_t)(nnodes1 + 1), 4 * (size_t)(mn + 1));
    const int a_f1 = H.in(feat1, 4 * (size_t)node_start1[nnodes1], 4 * (size_t)mx), a_v1 = H.in(valid1, (size_t)n1, (size_t)mx);
    const int a_i2 = H.in(node_ids2, 4 * (size_t)nnodes2, 4 * (size_t)mn), a_s2 = H.in(node_start2, 4 * (size_t)(nnodes2 + 1), 4 * (size_t)(mn + 1));
    const int a_f2 = H.in(feat2, 4 * (size_t)node_start2[nnodes2], 4 * (size_t)mx), a_v2 = H.in(valid2, (size_t)n2, (size_t)mx);
    const int a_k1 = H.in(kp1, sizeof(orbhip_keypoint) * (size_t)n1, sizeof(orbhip_keypoint) * (size_t)mx), a_k2 = H.in(kp2, sizeof(orbhip_keypoint) * (size_t)n2, sizeof(orbhip_keypoint) * (size_t)mx);
    const int a_d1 = H.in(desc1, 32 * (size_t)n1, 32 * (size_t)mx), a_d2 = H.in(desc2, 32 * (size_t)n2, 32 * (size_t)mx);
    const int a_nn1 = H.in(&nnodes1, 4), a_nn2 = H.in(&nnodes2, 4), a_n1 = H.in(&n1, 4), a_n2 = H.in(&n2, 4);
    const int a_m = H.out(matches12_out, 4 * (size_t)n1, 4 * (size_t)mx), a_nm = H.out(nmatches_out, 4);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_search_by_bow_kf_device(ctx, H.ptr<int32_t>(a_i1), H.ptr<int32_t>(a_s1), H.ptr<int32_t>(a_f1), H.ptr<int32_t>(a_nn1), H.ptr<uint8_t>(a_v1),
        H.ptr<orbhip_keypoint>(a_k1), H.ptr<uint8_t>(a_d1), H.ptr<int32_t>(a_n1), H.ptr<int32_t>(a_i2), H.ptr<int32_t>(a_s2), H.ptr<int32_t>(a_f2), H.ptr<int32_t>(a_nn2),
        H.ptr<uint8_t>(a_v2), H.ptr<orbhip_keypoint>(a_k2), H.ptr<uint8_t>(a_d2), H.ptr<int32_t>(a_n2), 1, mn, mx, (size_t)mx, nn_ratio, check_orientation,
        H.ptr<int32_t>(a_m), H.ptr<int32_t>(a_nm));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_pose_optimization_host(orbhip_ctx *ctx, const double *Xw, const double *obs, const double *inv_sigma2, int n,
                                             double fx, double fy, double cx, double cy, double bf, const double *kb8_k,
                                             const orbhip_camera2 *cam2, const uint8_t *right,
                                             double *pose_inout, uint8_t *outlier_out, int32_t *n_inliers_out, int32_t *stats_out)
{
    if (!ctx || n < 0 || !pose_inout || !n_inliers_out || (n && (!Xw || !obs || !inv_sigma2 || !outlier_out))) return ORBHIP_E_BADARG;
    *n_inliers_out = 0;
    if (stats_out) stats_out[0] = stats_out[1] = stats_out[2] = stats_out[3] = 0;
    if (n == 0) return ORBHIP_OK;
    HostCall H(ctx);
    const int a_x = H.in(Xw, 24 * (size_t)n), a_o = H.in(obs, 24 * (size_t)n), a_w = H.in(inv_sigma2, 8 * (size_t)n), a_n = H.in(&n, 4);
    const int a_r = H.in(right, (size_t)n), a_p = H.inout(pose_inout, 56), a_out = H.out(outlier_out, n), a_ni = H.out(n_inliers_out, 4), a_st = H.out(stats_out, stats_out ? 16 : 0, 16);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_pose_optimization_device(ctx, H.ptr<double>(a_x), H.ptr<double>(a_o), H.ptr<double>(a_w), H.ptr<int32_t>(a_n), 1, n, fx, fy, cx, cy, bf,
                                                   kb8_k, cam2, right ? H.ptr<uint8_t>(a_r) : nullptr, H.ptr<double>(a_p), H.ptr<uint8_t>(a_out), H.ptr<int32_t>(a_ni),
                                                   H.ptr<int32_t>(a_st));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_pose_inertial_optimization_host(orbhip_ctx *ctx, int mode, int rec_init, const orbhip_pim_rig *rig, int n,
        const double *Xw, const double *obs, const double *inv_sigma2, const uint8_t *kind, const uint8_t *close,
        const double *prev, const double *preint, const double *info, const double *info_g, const double *info_a,
        const double *prior, double *state_inout, uint8_t *outlier_out, int32_t *ret_out, double *H_out, int32_t *stats_out)
{
    if (!ctx || !rig || n < 0 || !prev || !preint || !info || !info_g || !info_a || (mode == 1 && !prior) || !state_inout || !ret_out ||
        !H_out || (n && (!Xw || !obs || !inv_sigma2 || !kind || !outlier_out)))
        return ORBHIP_E_BADARG;
    for (int i = 0; i < n; i++)                          // kind 2 needs the rig's second camera
        if (kind[i] > 2 || (kind[i] == 2 && !rig->has_cam2)) return ORBHIP_E_BADARG;
    HostCall H(ctx);
    const size_t ne = n > 0 ? (size_t)n : 1;
    const int a_x = H.in(Xw, 24 * (size_t)n, 24 * ne), a_o = H.in(obs, 24 * (size_t)n, 24 * ne), a_w = H.in(inv_sigma2, 8 * (size_t)n, 8 * ne);
    const int a_k = H.in(kind, (size_t)n, ne), a_c = H.in(close, (size_t)n, ne), a_n = H.in(&n, 4);
    const int a_pv = H.in(prev, 8 * ORBHIP_IBA_KF), a_pi = H.in(preint, 8 * ORBHIP_IBA_PREINT), a_i = H.in(info, 8 * 81);
    const int a_ig = H.in(info_g, 8 * 9), a_ia = H.in(info_a, 8 * 9), a_pr = H.in(prior, 8 * (ORBHIP_IBA_KF + 225));
    const int a_s = H.inout(state_inout, 8 * ORBHIP_IBA_KF), a_out = H.out(outlier_out, (size_t)n, ne), a_r = H.out(ret_out, 4);
    const int a_h = H.out(H_out, 8 * 225), a_st = H.out(stats_out, stats_out ? 16 : 0, 16);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_pose_inertial_optimization_device(ctx, mode, rec_init, rig, 1, n, H.ptr<double>(a_x), H.ptr<double>(a_o),
        H.ptr<double>(a_w), H.ptr<uint8_t>(a_k), close ? H.ptr<uint8_t>(a_c) : nullptr, H.ptr<int32_t>(a_n), H.ptr<double>(a_pv),
        H.ptr<double>(a_pi), H.ptr<double>(a_i), H.ptr<double>(a_ig), H.ptr<double>(a_ia), prior ? H.ptr<double>(a_pr) : nullptr,
        H.ptr<double>(a_s), H.ptr<uint8_t>(a_out), H.ptr<int32_t>(a_r), H.ptr<double>(a_h), H.ptr<int32_t>(a_st));
    if (rc) return rc;
    return H.finish();
}

// Optimizer::InertialOptimization for one map (host/Optimizer_InertialOptimization.cc); the trace travels both ways, so that rows of
// iterations that did not run keep the caller's content
extern "C" int orbhip_inertial_optimization_host(orbhip_ctx *ctx, const orbhip_inertial_opt_params *p, int n_kf, double *kf_inout,
        const uint8_t *link, const double *preint, const double *info, double *global_inout, double *stats_out, double *trace_out)
{
    if (!ctx || !p || n_kf < 0 || n_kf > 4096 || !global_inout || (n_kf && (!kf_inout || !link || !preint || !info)) || p->iterations < 0)
        return ORBHIP_E_BADARG;
    if (!p->free_vel_bias && !p->free_gdir && !p->free_scale) return ORBHIP_E_BADARG;
    const int32_t off[2] = {0, n_kf};
    const size_t n = (size_t)n_kf, ne = n ? n : 1, tb = trace_out ? 16 * (size_t)p->iterations : 0;
    HostCall H(ctx);
    const int a_off = H.in(off, 8), a_l = H.in(link, n, ne), a_p = H.in(preint, 8 * ORBHIP_IBA_PREINT * n, 8 * ORBHIP_IBA_PREINT * ne);
    const int a_i = H.in(info, 8 * 81 * n, 8 * 81 * ne);
    const int a_kf = H.inout(kf_inout, 8 * ORBHIP_IBA_KF * n, 8 * ORBHIP_IBA_KF * ne), a_g = H.inout(global_inout, 8 * ORBHIP_IO_GLOBAL);
    const int a_tr = H.inout(trace_out, tb, tb ? tb : 16);
    const int a_st = H.out(stats_out, stats_out ? 64 : 0, 64);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_inertial_optimization_device(ctx, p, 1, H.ptr<int32_t>(a_off), H.ptr<double>(a_kf), H.ptr<uint8_t>(a_l),
        H.ptr<double>(a_p), H.ptr<double>(a_i), H.ptr<double>(a_g), H.ptr<double>(a_st), trace_out ? H.ptr<double>(a_tr) : nullptr);
    if (rc) return rc;
    return H.finish();
}

// IMU::Preintegrated::Reintegrate / MergePrevious / ReintegrateBatch (host/ImuTypes.cc); the offsets are checked here, where they are
extern "C" int orbhip_preintegrate_host(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *meas_off, const float *meas,
        const uint8_t *cont, double *record_inout, float *cov_inout, float *avg_inout, double *info_out, double *info_g_out,
        double *info_a_out)
{
    if (int rc = orbhip_preint_check_args_internal(ctx, p, chains, meas_off, record_inout, cov_inout, avg_inout, info_out, info_g_out, info_a_out)) return rc;
    if (chains == 0) return ORBHIP_OK;
    if (int rc = orbhip_preint_check_offsets_internal(meas_off, chains, meas)) return rc;
    const size_t n = (size_t)chains, total = (size_t)meas_off[chains];
    const bool wi = p->want_info != 0;
    HostCall H(ctx);
    const int a_off = H.in(meas_off, 4 * (n + 1)), a_m = H.in(meas, 28 * total, 28 * (total ? total : 1)), a_c = H.in(cont, n, n);
    const int a_r = H.inout(record_inout, 8 * ORBHIP_IBA_PREINT * n), a_cv = H.inout(cov_inout, 4 * 225 * n), a_av = H.inout(avg_inout, 4 * 6 * n);
    const int a_i = H.out(info_out, wi ? 8 * 81 * n : 0, 8 * 81 * n), a_ig = H.out(info_g_out, wi ? 8 * 9 * n : 0, 8 * 9 * n);
    const int a_ia = H.out(info_a_out, wi ? 8 * 9 * n : 0, 8 * 9 * n);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_preint_launch_internal(ctx, p, chains, H.ptr<int32_t>(a_off), H.ptr<float>(a_m), cont ? H.ptr<uint8_t>(a_c) : nullptr,
        H.ptr<double>(a_r), H.ptr<float>(a_cv), H.ptr<float>(a_av), H.ptr<double>(a_i), H.ptr<double>(a_ig), H.ptr<double>(a_ia));
    if (rc) return rc;
    return H.finish();
}

// TwoViewReconstruction::Reconstruct for one frame pair (host/TwoViewReconstruction.cc)
extern "C" int orbhip_two_view_reconstruct_host(orbhip_ctx *ctx, const orbhip_keypoint *kp1, int n1, const orbhip_keypoint *kp2, int n2,
        const int32_t *matches12, float fx, float fy, float cx, float cy, const orbhip_tvr_params *p, int32_t *sets,
        uint8_t *ok_out, float *R21_out, float *t21_out, float *P3D_out, uint8_t *triangulated_out, orbhip_tvr_stats *stats_out)
{
    if (!ctx || n1 < 0 || n2 < 0 || !p || p->iterations <= 0 || !sets || !ok_out || !R21_out || !t21_out ||
        (n1 && (!kp1 || !matches12 || !P3D_out || !triangulated_out)) || (n2 && !kp2))
        return ORBHIP_E_BADARG;
    if (n1 > 8192 || n2 > 8192 || p->iterations > 1024) return ORBHIP_E_CAPACITY;
    const int max_n = n1 > n2 ? (n1 > 0 ? n1 : 1) : (n2 > 0 ? n2 : 1);
    const size_t kpb = sizeof(orbhip_keypoint), sb = 32 * (size_t)p->iterations;
    HostCall H(ctx);
    const int a_k1 = H.in(kp1, kpb * (size_t)n1, kpb * max_n), a_k2 = H.in(kp2, kpb * (size_t)n2, kpb * max_n);
    const int a_n1 = H.in(&n1, 4), a_n2 = H.in(&n2, 4), a_m = H.in(matches12, 4 * (size_t)n1, 4 * (size_t)max_n);
    const int a_s = p->draw_sets ? H.out(sets, sb) : H.inout(sets, sb);
    const int a_ok = H.out(ok_out, 1), a_R = H.out(R21_out, 36), a_t = H.out(t21_out, 12);
    const int a_P = H.out(P3D_out, 12 * (size_t)n1, 12 * (size_t)max_n), a_tr = H.out(triangulated_out, (size_t)n1, (size_t)max_n);
    const int a_st = H.out(stats_out, stats_out ? sizeof(orbhip_tvr_stats) : 0, sizeof(orbhip_tvr_stats));
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_two_view_reconstruct_device(ctx, H.ptr<orbhip_keypoint>(a_k1), H.ptr<int32_t>(a_n1), H.ptr<orbhip_keypoint>(a_k2),
        H.ptr<int32_t>(a_n2), (size_t)max_n, H.ptr<int32_t>(a_m), 1, max_n, fx, fy, cx, cy, p, H.ptr<int32_t>(a_s), H.ptr<uint8_t>(a_ok),
        H.ptr<float>(a_R), H.ptr<float>(a_t), H.ptr<float>(a_P), H.ptr<uint8_t>(a_tr), H.ptr<orbhip_tvr_stats>(a_st), nullptr, nullptr);
    if (rc) return rc;
    return H.finish();
}

// Optimizer::OptimizeSim3 for one keyframe pair (host/Optimizer_OptimizeSim3.cc)
extern "C" int orbhip_optimize_sim3_host(orbhip_ctx *ctx, const double *P1c, const double *P2c, const double *obs1, const double *obs2,
        const double *inv_sigma2_1, const double *inv_sigma2_2, int n, const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2,
        double th2, int fix_scale, double *sim3_inout, uint8_t *flag_out, int32_t *n_in_out, int32_t *stats_out)
{
    if (!ctx || n < 0 || !cam1 || !cam2 || !sim3_inout || !n_in_out || (n && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !flag_out)))
        return ORBHIP_E_BADARG;
    if (n > 8192) return ORBHIP_E_CAPACITY;
    *n_in_out = 0;
    if (stats_out) stats_out[0] = stats_out[1] = stats_out[2] = stats_out[3] = 0;
    if (n == 0) return ORBHIP_OK;                        // no edges: the reference returns 0 and leaves g2oS12 alone
    HostCall H(ctx);
    const size_t m = (size_t)n;
    const int a_p1 = H.in(P1c, 24 * m), a_p2 = H.in(P2c, 24 * m), a_o1 = H.in(obs1, 16 * m), a_o2 = H.in(obs2, 16 * m);
    const int a_w1 = H.in(inv_sigma2_1, 8 * m), a_w2 = H.in(inv_sigma2_2, 8 * m), a_n = H.in(&n, 4);
    const int a_s = H.inout(sim3_inout, 64), a_f = H.out(flag_out, m), a_ni = H.out(n_in_out, 4), a_st = H.out(stats_out, stats_out ? 16 : 0, 16);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_optimize_sim3_device(ctx, H.ptr<double>(a_p1), H.ptr<double>(a_p2), H.ptr<double>(a_o1), H.ptr<double>(a_o2),
        H.ptr<double>(a_w1), H.ptr<double>(a_w2), H.ptr<int32_t>(a_n), 1, n, cam1, cam2, th2, fix_scale, H.ptr<double>(a_s), H.ptr<uint8_t>(a_f),
        H.ptr<int32_t>(a_ni), H.ptr<int32_t>(a_st));
    if (rc) return rc;
    return H.finish();
}

// Sim3Solver for one candidate (host/Sim3Solver.cc)
extern "C" int orbhip_sim3_solver_host(orbhip_ctx *ctx, const float *X1c, const float *X2c, const float *max_err1, const float *max_err2, int n,
        const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2, const orbhip_sim3solver_params *p, int32_t *sets,
        uint8_t *converged_out, float *R12_out, float *t12_out, float *s12_out, int32_t *n_inliers_out, uint8_t *inlier_out,
        int32_t *stats_out, int32_t *counts_out)
{
    if (!ctx || n < 0 || !cam1 || !cam2 || !p || !sets || !converged_out || !R12_out || !t12_out || !s12_out || !n_inliers_out ||
        (n && (!X1c || !X2c || !max_err1 || !max_err2 || !inlier_out)))
        return ORBHIP_E_BADARG;
    if (n > 8192) return ORBHIP_E_CAPACITY;
    if (p->max_iterations < 1 || p->max_iterations > 1024)                       // the device form names the field
        return orbhip_sim3_solver_device(ctx, X1c, X2c, max_err1, max_err2, &n, 1, n > 0 ? n : 1, cam1, cam2, p, sets, converged_out, R12_out, t12_out,
                                         s12_out, n_inliers_out, inlier_out ? inlier_out : converged_out, stats_out, counts_out);
    const int max_n = n > 0 ? n : 1;
    const size_t m = (size_t)n, sb = 12 * (size_t)p->max_iterations, cb = 4 * (size_t)p->max_iterations;
    HostCall H(ctx);
    const int a_x1 = H.in(X1c, 12 * m, 12 * (size_t)max_n), a_x2 = H.in(X2c, 12 * m, 12 * (size_t)max_n);
    const int a_m1 = H.in(max_err1, 4 * m, 4 * (size_t)max_n), a_m2 = H.in(max_err2, 4 * m, 4 * (size_t)max_n), a_n = H.in(&n, 4);
    const int a_s = p->draw_sets ? H.out(sets, sb) : H.inout(sets, sb);
    const int a_R = H.inout(R12_out, 36), a_t = H.inout(t12_out, 12), a_sc = H.inout(s12_out, 4);      // untouched when n < min_inliers
    const int a_cv = H.out(converged_out, 1), a_ni = H.out(n_inliers_out, 4), a_in = H.out(inlier_out, m, (size_t)max_n);
    const int a_st = H.out(stats_out, stats_out ? 12 : 0, 12), a_ct = H.out(counts_out, counts_out ? cb : 0, cb);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_sim3_solver_device(ctx, H.ptr<float>(a_x1), H.ptr<float>(a_x2), H.ptr<float>(a_m1), H.ptr<float>(a_m2), H.ptr<int32_t>(a_n),
        1, max_n, cam1, cam2, p, H.ptr<int32_t>(a_s), H.ptr<uint8_t>(a_cv), H.ptr<float>(a_R), H.ptr<float>(a_t), H.ptr<float>(a_sc),
        H.ptr<int32_t>(a_ni), H.ptr<uint8_t>(a_in), H.ptr<int32_t>(a_st), counts_out ? H.ptr<int32_t>(a_ct) : nullptr);
    if (rc) return rc;
    return H.finish();
}

// MLPnPsolver for one candidate (host/MLPnPsolver.cc)
extern "C" int orbhip_mlpnp_solver_host(orbhip_ctx *ctx, const float *Xw, const float *p2d, const float *sigma2, int n, const orbhip_sim3_camera *cam,
        const orbhip_mlpnp_params *p, int32_t *sets, uint8_t *outcome_out, float *Tcw_out, int32_t *n_inliers_out, uint8_t *inlier_out,
        int32_t *stats_out, int32_t *counts_out)
{
    if (!ctx || n < 0 || !cam || !p || !sets || !outcome_out || !Tcw_out || !n_inliers_out || (n && (!Xw || !p2d || !sigma2 || !inlier_out)))
        return ORBHIP_E_BADARG;
    if (int rc = orbhip_mlpnp_check_params_internal(p, n)) return rc;             // the device form's rules, the field named, before anything is staged
    const int max_n = n > 0 ? n : 1;
    const size_t m = (size_t)n, sb = 24 * (size_t)p->max_iterations, cb = 4 * (size_t)p->max_iterations;
    HostCall H(ctx);
    const int a_x = H.in(Xw, 12 * m, 12 * (size_t)max_n), a_p = H.in(p2d, 8 * m, 8 * (size_t)max_n), a_s2 = H.in(sigma2, 4 * m, 4 * (size_t)max_n);
    const int a_n = H.in(&n, 4);
    const int a_s = p->draw_sets ? H.out(sets, sb) : H.inout(sets, sb);
    const int a_T = H.inout(Tcw_out, 48);                                        // untouched on outcome 0
    const int a_oc = H.out(outcome_out, 1), a_ni = H.out(n_inliers_out, 4), a_in = H.out(inlier_out, m, (size_t)max_n);
    const int a_st = H.out(stats_out, stats_out ? 16 : 0, 16), a_ct = H.out(counts_out, counts_out ? cb : 0, cb);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_mlpnp_solver_device(ctx, H.ptr<float>(a_x), H.ptr<float>(a_p), H.ptr<float>(a_s2), H.ptr<int32_t>(a_n), 1, max_n, cam, p,
        H.ptr<int32_t>(a_s), H.ptr<uint8_t>(a_oc), H.ptr<float>(a_T), H.ptr<int32_t>(a_ni), H.ptr<uint8_t>(a_in), H.ptr<int32_t>(a_st),
        counts_out ? H.ptr<int32_t>(a_ct) : nullptr);
    if (rc) return rc;
    return H.finish();
}

// Tracking::SearchLocalPoints for one frame (host/Tracking_SearchLocalPoints.cc): the frame record, the points and the train side go up in
// the blob, the frustum kernel and the matcher run on it back to back, the track records, the owner map and the claims come back
static int slp_host(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, const orbhip_local_points *pts, const orbhip_keypoint *kp, const uint8_t *desc,
                    const orbhip_keypoint *d_kp_res, const uint8_t *d_desc_res, const float *u_right, int n, int nleft, const int32_t *mirror,
                    float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio, orbhip_track_record *track_out,
                    int32_t *n_to_match_out, int32_t *owner_out, int32_t *nq_out, int32_t *train_match_inout, int32_t *nmatches_out)
{
    if (!ctx || !frame || !pts || !n_to_match_out || !nq_out || !nmatches_out) {
        orbhip_set_last_error_internal("orbhip_search_local_points_host: ctx, frame, points or a count output is NULL");
        return ORBHIP_E_BADARG;
    }
    if (pts->n != frame->n_points) { orbhip_set_last_error_internal("orbhip_search_local_points_host: points->n differs from frame->n_points"); return ORBHIP_E_BADARG; }
    const int np = pts->n;
    if (np < 0 || n < 0) { orbhip_set_last_error_internal("orbhip_search_local_points_host: a negative count (points->n, n)"); return ORBHIP_E_BADARG; }
    if (np && (!pts->Xw || !pts->normal || !pts->min_dist || !pts->max_dist || !pts->flags || !pts->desc || !track_out || !owner_out)) {
        orbhip_set_last_error_internal("orbhip_search_local_points_host: a per-point array (Xw, normal, min_dist, max_dist, flags, desc, track_out, owner_out) is NULL");
        return ORBHIP_E_BADARG;
    }
    if (n && ((!kp && !d_kp_res) || (!desc && !d_desc_res) || !train_match_inout)) {
        orbhip_set_last_error_internal("orbhip_search_local_points_host: a train-side array (kp, desc, train_match_inout) is NULL");
        return ORBHIP_E_BADARG;
    }
    if (nleft > n) { orbhip_set_last_error_internal("orbhip_search_local_points_host: nleft > n"); return ORBHIP_E_BADARG; }
    const bool rig = nleft >= 0;
    const int mp = np > 0 ? np : 1, mq = rig ? 2 * mp : mp, mn = n > 0 ? n : 1;
    if (int rc = orbhip_local_points_check_internal(frame, 1, mp, mq, rig, u_right != nullptr, mn, (size_t)mn, min_x, min_y, max_x, max_y)) return rc;
    *n_to_match_out = 0; *nq_out = 0; *nmatches_out = 0;
    if (np == 0) return ORBHIP_OK;
    const size_t P = (size_t)np;
    HostCall H(ctx);
    const int a_f = H.in(frame, sizeof(orbhip_frustum_frame));
    const int a_x = H.in(pts->Xw, 12 * P), a_nr = H.in(pts->normal, 12 * P), a_mi = H.in(pts->min_dist, 4 * P), a_ma = H.in(pts->max_dist, 4 * P);
    const int a_fl = H.in(pts->flags, P), a_pd = H.in(pts->desc, 32 * P), a_td = H.in(pts->track_depth, 4 * P);
    const int a_kp = H.in(d_kp_res ? nullptr : kp, sizeof(orbhip_keypoint) * (size_t)n, sizeof(orbhip_keypoint)), a_d = H.in(d_desc_res ? nullptr : desc, 32 * (size_t)n, 32);
    const int a_ur = H.in(u_right, 4 * (size_t)n), a_mr = H.in(rig ? mirror : nullptr, 4 * (size_t)n);
    const int a_n = H.in(&n, 4), a_nl = H.in(&nleft, 4);
    const int a_tm = H.inout(train_match_inout, 4 * (size_t)n, 4);
    const int a_tr = H.out(track_out, sizeof(orbhip_track_record) * P), a_nm = H.out(n_to_match_out, 4), a_ow = H.out(owner_out, 4 * (size_t)mq);
    const int a_nq = H.out(nq_out, 4), a_nmt = H.out(nmatches_out, 4);
    const int a_q = H.buf(sizeof(orbhip_proj_query) * (size_t)mq), a_dq = H.buf(32 * (size_t)mq);
    if (int rc = H.commit()) return rc;
    int rc;
    if (n == 0) {                                        // a frame without keypoints: nothing to match against
        ORB_HIP_TRY(hipMemsetAsync(H.ptr<int32_t>(a_nmt), 0, 4, H.s));
        rc = orbhip_frustum_launch_internal(ctx, H.ptr<orbhip_frustum_frame>(a_f), 1, mp, H.ptr<float>(a_x), H.ptr<float>(a_nr), H.ptr<float>(a_mi), H.ptr<float>(a_ma),
                                            H.ptr<uint8_t>(a_fl), H.ptr<uint8_t>(a_pd), pts->track_depth ? H.ptr<float>(a_td) : nullptr, min_x, min_y, max_x, max_y, mq,
                                            H.ptr<orbhip_track_record>(a_tr), H.ptr<int32_t>(a_nm), H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq),
                                            H.ptr<int32_t>(a_ow), H.ptr<int32_t>(a_nq));
    } else
        rc = orbhip_local_points_chain_internal(ctx, H.ptr<orbhip_frustum_frame>(a_f), 1, mp, H.ptr<float>(a_x), H.ptr<float>(a_nr), H.ptr<float>(a_mi),
                                                H.ptr<float>(a_ma), H.ptr<uint8_t>(a_fl), H.ptr<uint8_t>(a_pd), pts->track_depth ? H.ptr<float>(a_td) : nullptr, mq,
                                                d_kp_res ? d_kp_res : H.ptr<orbhip_keypoint>(a_kp), d_desc_res ? d_desc_res : H.ptr<uint8_t>(a_d),
                                                u_right ? H.ptr<float>(a_ur) : nullptr, H.ptr<int32_t>(a_n), rig ? H.ptr<int32_t>(a_nl) : nullptr,
                                                rig && mirror ? H.ptr<int32_t>(a_mr) : nullptr, mn, (size_t)mn, min_x, min_y, max_x, max_y, th_high, nn_ratio,
                                                H.ptr<orbhip_track_record>(a_tr), H.ptr<int32_t>(a_nm), H.ptr<orbhip_proj_query>(a_q), H.ptr<uint8_t>(a_dq),
                                                H.ptr<int32_t>(a_ow), H.ptr<int32_t>(a_nq), H.ptr<int32_t>(a_tm), H.ptr<int32_t>(a_nmt));
    if (rc) return rc;
    return H.finish();
}

extern "C" int orbhip_search_local_points_host(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, const orbhip_local_points *points,
        const orbhip_keypoint *kp, const uint8_t *desc, const float *u_right, int n, int nleft, const int32_t *mirror,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio, orbhip_track_record *track_out,
        int32_t *n_to_match_out, int32_t *owner_out, int32_t *nq_out, int32_t *train_match_inout, int32_t *nmatches_out)
{
    return slp_host(ctx, frame, points, kp, desc, nullptr, nullptr, u_right, n, nleft < 0 ? -1 : nleft, mirror, min_x, min_y, max_x, max_y, th_high, nn_ratio,
                    track_out, n_to_match_out, owner_out, nq_out, train_match_inout, nmatches_out);
}

extern "C" int orbhip_search_local_points_host_resident(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, const orbhip_local_points *points,
        const orbhip_keypoint *kp_host, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *u_right, int n,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio, orbhip_track_record *track_out,
        int32_t *n_to_match_out, int32_t *owner_out, int32_t *nq_out, int32_t *train_match_inout, int32_t *nmatches_out)
{
    if (n && (!d_desc || (!d_kp && !kp_host))) { orbhip_set_last_error_internal("orbhip_search_local_points_host_resident: d_desc, or both d_kp and kp_host, NULL"); return ORBHIP_E_BADARG; }
    return slp_host(ctx, frame, points, d_kp ? nullptr : kp_host, nullptr, d_kp, d_desc, u_right, n, -1, nullptr, min_x, min_y, max_x, max_y, th_high, nn_ratio,
                    track_out, n_to_match_out, owner_out, nq_out, train_match_inout, nmatches_out);
}

// KeyFrameDatabase: one query against the device-resident database (host/KeyFrameDatabase.cc): the query record, its vector and its
// connected slots go up in the blob, the counts and the sharing list come back
extern "C" int orbhip_kfdb_score_host(orbhip_kfdb *db, const orbhip_kfdb_query *query, const int32_t *word, const double *value, int nwords,
        const int32_t *connected, int n_connected, int max_list, int32_t *counts_out, orbhip_kfdb_entry *list_out)
{
    if (!db) { orbhip_set_last_error_internal("orbhip_kfdb_score_host: db is NULL"); return ORBHIP_E_BADARG; }
    if (!query || !counts_out || !list_out) { orbhip_set_last_error_internal("orbhip_kfdb_score_host: query, counts_out or list_out is NULL"); return ORBHIP_E_BADARG; }
    if (nwords < 0 || n_connected < 0 || (nwords && (!word || !value)) || (n_connected && !connected)) {
        orbhip_set_last_error_internal("orbhip_kfdb_score_host: a negative count (nwords, n_connected) or a NULL array behind a positive one");
        return ORBHIP_E_BADARG;
    }
    if (nwords > orbhip_kfdb_max_words_internal(db)) { orbhip_set_last_error_internal("orbhip_kfdb_score_host: nwords > max_words"); return ORBHIP_E_CAPACITY; }
    if (max_list < 1 || max_list > ORBHIP_KFDB_MAX_LIST) { orbhip_set_last_error_internal("orbhip_kfdb_score_host: max_list outside 1..4096"); return ORBHIP_E_CAPACITY; }
    orbhip_ctx *ctx = orbhip_kfdb_ctx_internal(db);
    const int stride = nwords > 0 ? nwords : 1, mc = n_connected > 0 ? n_connected : 1;
    HostCall H(ctx);
    const int a_q = H.in(query, sizeof(orbhip_kfdb_query)), a_w = H.in(word, 4 * (size_t)nwords, 4 * (size_t)stride), a_v = H.in(value, 8 * (size_t)nwords, 8 * (size_t)stride);
    const int a_n = H.in(&nwords, 4), a_c = H.in(connected, 4 * (size_t)n_connected, 4 * (size_t)mc), a_nc = H.in(&n_connected, 4);
    const int a_cnt = H.out(counts_out, 16), a_l = H.out(list_out, sizeof(orbhip_kfdb_entry) * (size_t)max_list);
    if (int rc = H.commit()) return rc;
    const int rc = orbhip_kfdb_launch_internal(db, "orbhip_kfdb_score_host", query, H.ptr<orbhip_kfdb_query>(a_q), 1, H.ptr<int32_t>(a_w), H.ptr<double>(a_v),
        H.ptr<int32_t>(a_n), stride, H.ptr<int32_t>(a_c), H.ptr<int32_t>(a_nc), mc, nullptr, 0, nullptr, 0, max_list, H.ptr<int32_t>(a_cnt),
        H.ptr<orbhip_kfdb_entry>(a_l), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    return H.finish();
}
