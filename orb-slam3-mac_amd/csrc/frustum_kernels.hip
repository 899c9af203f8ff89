// frustum_kernels.hip -- Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:483-572, :1170-1243) over the local map points of a
// frame, and the query list ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) builds from what they leave in
// the MapPoints (src/ORBmatcher.cc:54-79, :149-156): the host loop in front of the local-map matcher (Tracking::SearchLocalPoints,
// src/Tracking.cc:2380-2429), so that a list of points goes in and the matcher's queries come out on the same stream.
//
// One workgroup of ORBHIP_FRUSTUM_CHUNK lanes per frame; the points go through it a chunk at a time.  A lane does all the geometry of its
// point first (both cameras of a rig), then the chunk's queries are numbered in LIST order -- the claim rule of the matcher depends on
// it: prefix inside a wave from two ballots (left query, right query), the wave totals through LDS, two barriers per chunk -- and the
// lane writes its queries, gathers its descriptor (two 16-byte loads, two 16-byte stores per query) and names itself their owner.
//
// Arithmetic, op by op (the file is compiled -ffp-contract=off; roundings as host/cvmath.h documents them for OpenCV):
//   Pc = R*P + t        cv::gemm's small-matrix path: the row's products summed in float, then (float)((double)sum + (double)t)
//   cv::norm, Mat::dot  accumulated in double; Pc_dist / dist = (float)sqrt(sum), viewCos = (float)(dot / (double)dist)
//   P - Ow              a float subtraction per element
//   project             tri_project of cam_project_f32.h
// The comparisons are the reference's own, not their negations: a NaN projection (PcZ == 0 and x == 0 through a pinhole) passes the
// bounds tests as it does there, and PcZ == -0.0f is not negative.
// MapPoint::PredictScale (src/MapPoint.cc:514-546) without a device logarithm: the host finds, with ITS logf, the smallest ratio of every
// level (orbhip_predict_scale_thresholds below) and the kernel counts the thresholds the ratio reaches.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "cam_project_f32.h"
#include <cmath>
#include <cstddef>
#include <cstring>

namespace {

constexpr int FR_THREADS = ORBHIP_FRUSTUM_CHUNK;
constexpr int FR_WAVES = FR_THREADS / 64;

struct FrArgs {
    const orbhip_frustum_frame *frame;
    const float *Xw, *normal, *min_dist, *max_dist, *track_depth;
    const uint8_t *flags, *desc;
    float min_x, min_y, max_x, max_y;
    int max_points, max_q;
    orbhip_track_record *track;
    int32_t *n_to_match, *owner, *nq, *status;
    orbhip_proj_query *q;
    uint8_t *desc_q;
};

static_assert(sizeof(orbhip_frustum_frame) == 480 && sizeof(orbhip_track_record) == 44 && sizeof(orbhip_proj_query) == 32, "record layouts (python/orbhip.py mirrors them)");
// the right camera's pose follows the left one's in the record: Rcw tcw Ow | Rrw trw Orw
constexpr int FR_POSE_STRIDE = 15;
static_assert(offsetof(orbhip_frustum_frame, Rrw) == offsetof(orbhip_frustum_frame, Rcw) + 4 * FR_POSE_STRIDE && offsetof(orbhip_frustum_frame, trw) == offsetof(orbhip_frustum_frame, tcw) + 4 * FR_POSE_STRIDE &&
              offsetof(orbhip_frustum_frame, Orw) == offsetof(orbhip_frustum_frame, Ow) + 4 * FR_POSE_STRIDE, "orbhip_frustum_frame: pose layout");

struct FrCam { float u, v, depth, view_cos, invz; int level; };

// Frame::isInFrustumChecks for one camera (and lines :497-541 of the single-camera branch, which are the same tests): the outcome code
static __device__ int fr_camera(const float *R, const float *t, const float *O, int type, const float *cam, const float *X, const float *N,
                                float min_raw, float max_raw, const FrArgs &a, const orbhip_frustum_frame *f, FrCam &o)
{
    float Pc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float s = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2];
        Pc[i] = (float)((double)s + (double)t[i]);
    }
    o.depth = (float)sqrt((double)Pc[0] * (double)Pc[0] + (double)Pc[1] * (double)Pc[1] + (double)Pc[2] * (double)Pc[2]);
    o.invz = 1.0f / Pc[2];
    // every test is evaluated for every point and the first one that fails names the outcome: the tests are a few dozen operations, and
    // a lane that left early would only wait for its neighbours (what a rejected point computes past its test is never stored)
    float uv[2];
    tri_project(type, cam, Pc, uv);
    const float PO[3] = {X[0] - O[0], X[1] - O[1], X[2] - O[2]};
    const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
    const double dot = (double)PO[0] * (double)N[0] + (double)PO[1] * (double)N[1] + (double)PO[2] * (double)N[2];
    const float view_cos = (float)(dot / (double)dist);
    // PredictScale: the clamped level is the number of level thresholds the ratio reaches; undefined inputs of the reference give 0
    const float ratio = max_raw / dist;
    int level = 0;
    for (int n = 0; n < f->nlevels - 1; n++) level += ratio >= f->level_thresholds[n] ? 1 : 0;
    if (!(ratio > 0.0f && ratio < INFINITY)) level = 0;
    int code = 0;
    if (view_cos < f->viewing_cos_limit) code = 7;                                // Frame.cc:537, :1221
    if (dist > 1.2f * max_raw) code = 6;                                          // :525, :1213
    if (dist < 0.8f * min_raw) code = 5;
    if (uv[1] < a.min_y || uv[1] > a.max_y) code = 4;                             // :512, :1204
    if (uv[0] < a.min_x || uv[0] > a.max_x) code = 3;                             // :510, :1202
    if (Pc[2] < 0.0f) code = 2;                                                   // :503, :1194
    o.u = uv[0]; o.v = uv[1]; o.view_cos = view_cos; o.level = level;
    return code;
}

static __device__ __forceinline__ void fr_emit(const FrArgs &a, size_t qrow, int slot, float u, float v, float radius, float ur, int level, int has_obs,
                                               uint4 d0, uint4 d1, int owner)
{
    float4 *Q = reinterpret_cast<float4 *>(a.q + qrow + slot);                    // orbhip_proj_query: 32 bytes, two 16-byte stores
    Q[0] = make_float4(u, v, radius, ur);
    Q[1] = make_float4(0.0f, __int_as_float(level - 1), __int_as_float(level), __int_as_float(has_obs));
    uint4 *D = reinterpret_cast<uint4 *>(a.desc_q + (qrow + slot) * 32);
    D[0] = d0; D[1] = d1;
    a.owner[qrow + slot] = owner;
}

__global__ __launch_bounds__(FR_THREADS) void k_frustum_queries(FrArgs args)
{
    __shared__ int s_q[FR_WAVES], s_m[FR_WAVES];
    const int frame = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                  // uniform in a wave: the compares against it below are scalar
    // the frame's record and the kernel's own arguments are read through LDS where they are used: held in scalar registers for the whole
    // chunk loop (~60 words of the record, 17 pointers) beside the constants of the double atan2 / sincos sequences, they did not fit
    // (the resource listing showed scalar registers spilled into vector lanes)
    __shared__ orbhip_frustum_frame s_f;
    __shared__ FrArgs s_a;
    if (tid == 0) s_a = args;
    const FrArgs &a = s_a;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(args.frame + frame);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&s_f);
        for (int k = tid; k < (int)(sizeof(orbhip_frustum_frame) / 4); k += FR_THREADS) dst[k] = src[k];
    }
    __syncthreads();
    const orbhip_frustum_frame *f = &s_f;
    const int np = f->n_points, rig = f->rig != 0;
    const size_t row = (size_t)frame * a.max_points, qrow = (size_t)frame * a.max_q;
    const float th = f->th;
    int base = 0, to_match = 0;                                                   // uniform over the workgroup
    for (int c0 = 0; c0 < np; c0 += FR_THREADS) {
        const int i = c0 + tid;
        bool ql = false, qr = false, seen = false;
        FrCam L, Rr;
        int has_obs = 0;
        if (i < np) {
            const uint8_t flag = a.flags[row + i];
            has_obs = flag & 1;
            orbhip_track_record rec;
            rec.proj_x = rec.proj_y = rec.proj_xr = rec.proj_yr = rec.depth = rec.depth_r = rec.view_cos = rec.view_cos_r = 0.0f;
            rec.level = rec.level_r = rig ? -1 : 0;
            rec.in_view = rec.in_view_r = 0; rec.code = 1; rec.code_r = rig ? 1 : 255;
            if (!(flag & 2)) {
                const float *Xp = a.Xw + 3 * (row + i), *Np = a.normal + 3 * (row + i);
                const float X[3] = {Xp[0], Xp[1], Xp[2]}, N[3] = {Np[0], Np[1], Np[2]};
                const float min_raw = a.min_dist[row + i], max_raw = a.max_dist[row + i];
                // one camera per trip, not unrolled: only one camera's pose and parameters are live at a time (scalar registers)
                int cl = 1, cr = 1;
#pragma unroll 1
                for (int c = 0; c <= rig; c++) {
                    FrCam o;
                    const int code = fr_camera(f->Rcw + FR_POSE_STRIDE * c, f->tcw + FR_POSE_STRIDE * c, f->Ow + FR_POSE_STRIDE * c, f->cam_type[c], f->cam[c],
                                               X, N, min_raw, max_raw, a, f, o);
                    if (c == 0) { L = o; cl = code; } else { Rr = o; cr = code; }
                }
                rec.code = (uint8_t)cl;
                float far_depth = a.track_depth ? a.track_depth[row + i] : 0.0f;  // mTrackDepth as ORBmatcher.cc:60 will find it
                if (!rig) {                                                       // Frame.cc:485-560
                    rec.proj_x = rec.proj_y = -1.0f;
                    if (cl == 0 || cl >= 5) { rec.proj_x = L.u; rec.proj_y = L.v; }
                    if (cl == 0) {
                        rec.in_view = 1; rec.proj_xr = L.u - f->mbf * L.invz; rec.depth = L.depth; rec.level = L.level; rec.view_cos = L.view_cos;
                        far_depth = L.depth;
                    }
                } else {                                                          // :562-570
                    if (cl == 0) {
                        rec.in_view = 1; rec.proj_x = L.u; rec.proj_y = L.v; rec.level = L.level; rec.view_cos = L.view_cos; rec.depth = L.depth;
                        far_depth = L.depth;
                    }
                    rec.code_r = (uint8_t)cr;
                    if (cr == 0) { rec.in_view_r = 1; rec.proj_xr = Rr.u; rec.proj_yr = Rr.v; rec.level_r = Rr.level; rec.view_cos_r = Rr.view_cos; rec.depth_r = Rr.depth; }
                }
                seen = rec.in_view || rec.in_view_r;
                const bool far = f->far_points && far_depth > f->th_far_points;   // ORBmatcher.cc:60
                ql = rec.in_view && !far;
                qr = rec.in_view_r && !far;                                       // (its level is never -1 here: ORBmatcher.cc:151)
            }
            a.track[row + i] = rec;
            L.u = rec.proj_x; L.v = rec.proj_y; L.invz = rec.proj_xr;             // the left query's u, v, ur
        }
        const unsigned long long bl = __ballot(ql), br = __ballot(qr), bs = __ballot(seen);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int pre = __popcll(bl & below) + __popcll(br & below);
        if (lane == 0) { s_q[wave] = __popcll(bl) + __popcll(br); s_m[wave] = __popcll(bs); }
        __syncthreads();
        int slot = base + pre, total = 0;
#pragma unroll
        for (int w = 0; w < FR_WAVES; w++) { const int t = s_q[w]; if (w < wave) slot += t; total += t; to_match += s_m[w]; }
        __syncthreads();                                                          // the totals are read before the next chunk stores its own
        base += total;
        if (ql || qr) {
            const uint4 *D = reinterpret_cast<const uint4 *>(a.desc + (row + i) * 32);
            const uint4 d0 = D[0], d1 = D[1];
            if (ql) {
                if (slot < a.max_q) {
                    float r = (double)L.view_cos > 0.998 ? 2.5f : 4.0f;          // ORBmatcher::RadiusByViewingCos
                    if (th != 1.0f) r *= th;
                    fr_emit(a, qrow, slot, L.u, L.v, r * f->scale_factors[L.level], L.invz, L.level, has_obs, d0, d1, i);
                }
                slot++;
            }
            if (qr && slot < a.max_q) {
                const float r = (double)Rr.view_cos > 0.998 ? 2.5f : 4.0f;
                fr_emit(a, qrow, slot, Rr.u, Rr.v, r * f->scale_factors[Rr.level], -1.0f, Rr.level, has_obs | 2, d0, d1, i);
            }
        }
    }
    if (tid == 0) {
        a.n_to_match[frame] = to_match;
        if (base > a.max_q) { atomicExch(a.status, ORBHIP_E_CAPACITY); base = 0; }
        a.nq[frame] = base;
    }
}

}  // namespace

extern "C" int orbhip_frustum_chunk(void) { return ORBHIP_FRUSTUM_CHUNK; }

// ceil(log(ratio) / mfLogScaleFactor) > n, the expression of MapPoint::PredictScale with the caller's libm (compared in float: the
// conversion to int is undefined for the few huge quotients a tiny scale factor could give, and equal wherever it is defined)
static bool fr_level_exceeds(float ratio, float log_scale_factor, int n) { return std::ceil(std::log(ratio) / log_scale_factor) > (float)n; }

extern "C" int orbhip_predict_scale_thresholds(float log_scale_factor, int nlevels, float *out)
{
    if (!out) { orbhip_set_last_error_internal("orbhip_predict_scale_thresholds: out is NULL"); return ORBHIP_E_BADARG; }
    if (nlevels < 1 || nlevels > ORBHIP_FRUSTUM_MAX_LEVELS) { orbhip_set_last_error_internal("orbhip_predict_scale_thresholds: nlevels outside 1..32"); return ORBHIP_E_BADARG; }
    if (!(log_scale_factor > 0.0f) || !(log_scale_factor < INFINITY)) {
        orbhip_set_last_error_internal("orbhip_predict_scale_thresholds: log_scale_factor is not a positive finite number");
        return ORBHIP_E_BADARG;
    }
    for (int n = 0; n < nlevels - 1; n++) {
        // positive floats are ordered as their bit patterns; the level does not decrease with the ratio
        uint32_t lo = 1u, hi = 0x7f7fffffu;                                       // smallest subnormal (level 0), largest finite float
        float v;
        memcpy(&v, &hi, 4);
        if (!fr_level_exceeds(v, log_scale_factor, n)) { out[n] = INFINITY; continue; }
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            memcpy(&v, &mid, 4);
            if (fr_level_exceeds(v, log_scale_factor, n)) hi = mid; else lo = mid;
        }
        memcpy(&out[n], &hi, 4);
    }
    return ORBHIP_OK;
}

// the checks every entry point makes on the HOST records before anything is launched
int orbhip_frustum_check_internal(const orbhip_frustum_frame *frame, int frames, int max_points, int max_q)
{
    if (frames <= 0) { orbhip_set_last_error_internal("frustum_queries: frames < 1"); return ORBHIP_E_BADARG; }
    if (max_points <= 0) { orbhip_set_last_error_internal("frustum_queries: max_points < 1"); return ORBHIP_E_BADARG; }
    if (max_q <= 0) { orbhip_set_last_error_internal("frustum_queries: max_q < 1"); return ORBHIP_E_BADARG; }
    for (int k = 0; k < frames; k++) {
        const orbhip_frustum_frame &f = frame[k];
        if (f.nlevels < 1 || f.nlevels > ORBHIP_FRUSTUM_MAX_LEVELS) { orbhip_set_last_error_internal("frustum_queries: nlevels outside 1..32"); return ORBHIP_E_BADARG; }
        if (f.n_points < 0 || f.n_points > max_points) { orbhip_set_last_error_internal("frustum_queries: n_points outside 0..max_points"); return ORBHIP_E_BADARG; }
        if ((f.cam_type[0] | 1) != 1) { orbhip_set_last_error_internal("frustum_queries: cam_type[0] is neither 0 (Pinhole) nor 1 (KannalaBrandt8)"); return ORBHIP_E_BADARG; }
        if (f.rig && (f.cam_type[1] | 1) != 1) {
            orbhip_set_last_error_internal("frustum_queries: cam_type[1]: a rig frame without a second camera (0 Pinhole, 1 KannalaBrandt8)");
            return ORBHIP_E_BADARG;
        }
    }
    return ORBHIP_OK;
}

// the launch: d_frame on the DEVICE, already checked
int orbhip_frustum_launch_internal(orbhip_ctx *ctx, const orbhip_frustum_frame *d_frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, float min_x, float min_y, float max_x, float max_y, int max_q,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq)
{
    FrArgs a;
    a.frame = d_frame; a.Xw = d_Xw; a.normal = d_normal; a.min_dist = d_min_dist; a.max_dist = d_max_dist; a.track_depth = d_track_depth;
    a.flags = d_flags; a.desc = d_desc; a.min_x = min_x; a.min_y = min_y; a.max_x = max_x; a.max_y = max_y;
    a.max_points = max_points; a.max_q = max_q; a.track = d_track; a.n_to_match = d_n_to_match; a.owner = d_owner; a.nq = d_nq;
    a.status = orbhip_ctx_status_internal(ctx); a.q = d_q; a.desc_q = d_desc_q;
    hipLaunchKernelGGL(k_frustum_queries, dim3(frames), dim3(FR_THREADS), 0, orbhip_ctx_stream_internal(ctx), a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_frustum_queries launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}

extern "C" int orbhip_frustum_queries_device(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, float min_x, float min_y, float max_x, float max_y, int max_q,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq)
{
    if (!ctx || !frame || !d_Xw || !d_normal || !d_min_dist || !d_max_dist || !d_flags || !d_desc || !d_track || !d_n_to_match || !d_q ||
        !d_desc_q || !d_owner || !d_nq) {
        orbhip_set_last_error_internal("orbhip_frustum_queries_device: a required pointer is NULL");
        return ORBHIP_E_BADARG;
    }
    if (int rc = orbhip_frustum_check_internal(frame, frames, max_points, max_q)) return rc;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    // the per-frame records go to the context's work arena (grow-only: a warmed-up context allocates nothing here).  The copy is ordered
    // on the stream behind an earlier call's kernels, which have read their own records by then; the caller's array is free on return
    const size_t bytes = (size_t)frames * sizeof(orbhip_frustum_frame);
    orbhip_frustum_frame *d_frame = (orbhip_frustum_frame *)orbhip_ctx_work_internal(ctx, align256(bytes));
    if (!d_frame) return ORBHIP_E_HIP;
    ORB_HIP_TRY(hipMemcpyAsync(d_frame, frame, bytes, hipMemcpyHostToDevice, orbhip_ctx_stream_internal(ctx)));
    return orbhip_frustum_launch_internal(ctx, d_frame, frames, max_points, d_Xw, d_normal, d_min_dist, d_max_dist, d_flags, d_desc, d_track_depth,
                                          min_x, min_y, max_x, max_y, max_q, d_track, d_n_to_match, d_q, d_desc_q, d_owner, d_nq);
}

// the matcher behind the frustum kernel, both on the context's stream (the records d_frame on the DEVICE; `rig` = what the checked host
// records say)
int orbhip_local_points_chain_internal(orbhip_ctx *ctx, const orbhip_frustum_frame *d_frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc_kp,
        const float *d_u_right, const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n, size_t frame_stride_kp,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq,
        int32_t *d_train_match, int32_t *d_nmatches)
{
    if (int rc = orbhip_frustum_launch_internal(ctx, d_frame, frames, max_points, d_Xw, d_normal, d_min_dist, d_max_dist, d_flags, d_desc, d_track_depth,
                                                min_x, min_y, max_x, max_y, max_q, d_track, d_n_to_match, d_q, d_desc_q, d_owner, d_nq)) return rc;
    if (d_nleft)
        return orbhip_search_by_projection_rig_device(ctx, 1, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc_kp, d_n, d_nleft, d_mirror, max_n, frame_stride_kp,
                                                      frames, min_x, min_y, max_x, max_y, th_high, nn_ratio, 0, d_train_match, d_nmatches);
    return orbhip_search_local_map_device(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc_kp, d_u_right, d_n, max_n, frame_stride_kp, frames,
                                          min_x, min_y, max_x, max_y, th_high, nn_ratio, d_train_match, d_nmatches);
}

int orbhip_local_points_check_internal(const orbhip_frustum_frame *frame, int frames, int max_points, int max_q, bool rig_train, bool has_u_right,
                                       int max_n, size_t frame_stride_kp, float min_x, float min_y, float max_x, float max_y)
{
    if (int rc = orbhip_frustum_check_internal(frame, frames, max_points, max_q)) return rc;
    if (max_n <= 0) { orbhip_set_last_error_internal("search_local_points: max_n < 1"); return ORBHIP_E_BADARG; }
    if (frame_stride_kp < (size_t)max_n) { orbhip_set_last_error_internal("search_local_points: frame_stride_kp < max_n"); return ORBHIP_E_BADARG; }
    if (!(max_x > min_x) || !(max_y > min_y)) { orbhip_set_last_error_internal("search_local_points: empty image bounds (min_x .. max_y)"); return ORBHIP_E_BADARG; }
    if (rig_train && has_u_right) { orbhip_set_last_error_internal("search_local_points: d_u_right with d_nleft (a rig frame has no uRight)"); return ORBHIP_E_BADARG; }
    for (int k = 0; k < frames; k++)
        if ((frame[k].rig != 0) != rig_train) {
            orbhip_set_last_error_internal("search_local_points: rig: a frame record and the train side (d_nleft) disagree");
            return ORBHIP_E_BADARG;
        }
    return ORBHIP_OK;
}

extern "C" int orbhip_search_local_points_device(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc_kp,
        const float *d_u_right, const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n, size_t frame_stride_kp,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq,
        int32_t *d_train_match, int32_t *d_nmatches)
{
    if (!ctx || !frame || !d_Xw || !d_normal || !d_min_dist || !d_max_dist || !d_flags || !d_desc || !d_track || !d_n_to_match || !d_q ||
        !d_desc_q || !d_owner || !d_nq || !d_kp || !d_desc_kp || !d_n || !d_train_match || !d_nmatches) {
        orbhip_set_last_error_internal("orbhip_search_local_points_device: a required pointer is NULL");
        return ORBHIP_E_BADARG;
    }
    if (int rc = orbhip_local_points_check_internal(frame, frames, max_points, max_q, d_nleft != nullptr, d_u_right != nullptr, max_n, frame_stride_kp,
                                                    min_x, min_y, max_x, max_y)) return rc;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    // the records share the work arena with the matcher's own buffers: the matcher's kernels start after the frustum kernel has ended
    // (one stream), and an arena that has to grow waits for the stream first
    const size_t bytes = (size_t)frames * sizeof(orbhip_frustum_frame);
    orbhip_frustum_frame *d_frame = (orbhip_frustum_frame *)orbhip_ctx_work_internal(ctx, align256(bytes));
    if (!d_frame) return ORBHIP_E_HIP;
    ORB_HIP_TRY(hipMemcpyAsync(d_frame, frame, bytes, hipMemcpyHostToDevice, orbhip_ctx_stream_internal(ctx)));
    return orbhip_local_points_chain_internal(ctx, d_frame, frames, max_points, d_Xw, d_normal, d_min_dist, d_max_dist, d_flags, d_desc, d_track_depth,
                                              max_q, d_kp, d_desc_kp, d_u_right, d_n, d_nleft, d_mirror, max_n, frame_stride_kp, min_x, min_y, max_x, max_y,
                                              th_high, nn_ratio, d_track, d_n_to_match, d_q, d_desc_q, d_owner, d_nq, d_train_match, d_nmatches);
}
