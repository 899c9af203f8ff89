// orbhip_api.hip -- C-ABI implementation: context + ORB extractor (include/orbhip.h).
// Host logic mirrors ORBextractor's constructor / ComputePyramid bookkeeping
// (reference src/ORBextractor.cc:408-468, 1152-1177) and owns all device memory.
#include "orb_internal.h"
#include "ctx_internal.h"
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <mutex>
#include <set>
#include <utility>

static thread_local std::string g_last_error;
extern "C" const char *orbhip_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *orbhip_version(void) { return "orbhip 0.1 (gfx950)"; }

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);           \
            return ORBHIP_E_HIP;                                                        \
        }                                                                               \
    } while (0)

int orb_lds_optin(const void *func, int device, size_t need)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    const size_t total = 160 * 1024;
    std::lock_guard<std::mutex> lk(mu);
    if (!done.count({func, device})) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, func) != hipSuccess) { g_last_error = "hipFuncGetAttributes"; return ORBHIP_E_HIP; }
        const int maxdyn = (int)(total - std::min(total, (size_t)fa.sharedSizeBytes));
        if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, maxdyn) != hipSuccess) { g_last_error = "hipFuncSetAttribute(MaxDynamicSharedMemorySize)"; return ORBHIP_E_HIP; }
        done.insert({func, device});
    }
    if (need > total) { g_last_error = "dynamic LDS request exceeds 160 KB"; return ORBHIP_E_BADARG; }
    return ORBHIP_OK;
}

struct orbhip_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    int32_t *d_status;      // sticky device-side error word (capacity overflows in matcher kernels)
    int32_t *status_redirect;
    void *scratch;          // grow-only device arena of the host-pointer convenience entry points (host_entry.hip)
    size_t scratch_bytes;
    void *work;             // grow-only device arena of the device entry points themselves (candidate lists of the low-latency matchers): separate from
    size_t work_bytes;      // `scratch`, which holds the host-form callers' staged inputs while those entry points run
    int n_cus;              // hipDeviceAttributeMultiprocessorCount of `device`: persistent grids are sized from it
    int ba_schur_mode;      // orbhip_ctx_set_ba_schur_mode
    void *ba_arena; size_t ba_arena_bytes; bool ba_arena_busy;     // cached device arena of one-shot local-BA solves (ba_kernels.hip)
    int *pinned_word;       // one page-locked word for such solves (the LM loop's active-graph counter)
    void *pinned;           // grow-only page-locked host arena of the host-pointer entry points: a call's inputs are gathered here and leave in ONE
    size_t pinned_bytes;    // host-to-device copy, its outputs come back in ONE device-to-host copy (host_entry.hip)
    size_t sbp_redo_off;    // the last SearchByProjection launch's per-pair hand-back flags: their offset in `work` and their number (0: that
    int sbp_redo_pairs;     // launch did not run the replay form) -- orbhip_debug_sbp_handed_back
};

extern "C" int orbhip_ctx_create(int device, void *stream, orbhip_ctx **out)
{
    if (!out) return ORBHIP_E_BADARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || device < 0 || device >= n) {
        g_last_error = "no HIP device (this library has no CPU fallback)";
        return ORBHIP_E_NODEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    orbhip_ctx *c = new orbhip_ctx();
    c->device = device;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        hipError_t e2 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e2 != hipSuccess) { delete c; g_last_error = hipGetErrorString(e2); return ORBHIP_E_HIP; }
        c->own_stream = true;
    }
    if (hipMalloc((void **)&c->d_status, sizeof(int32_t)) != hipSuccess || hipMemset(c->d_status, 0, sizeof(int32_t)) != hipSuccess) {
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        delete c; g_last_error = "hipMalloc(status)"; return ORBHIP_E_HIP;
    }
    c->status_redirect = nullptr;
    c->scratch = nullptr; c->scratch_bytes = 0; c->work = nullptr; c->work_bytes = 0; c->ba_schur_mode = 0; c->n_cus = 0; c->pinned = nullptr; c->pinned_bytes = 0; c->ba_arena = nullptr; c->ba_arena_bytes = 0; c->ba_arena_busy = false; c->pinned_word = nullptr;
    if (hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cus <= 0) c->n_cus = 256;
    *out = c;
    return ORBHIP_OK;
}
// Device arena of at least `bytes` (256-byte aligned), kept across calls; growing drains the stream first.
void *orbhip_ctx_scratch_internal(orbhip_ctx *c, size_t bytes)
{
    if (bytes <= c->scratch_bytes) return c->scratch;
    (void)hipStreamSynchronize(c->stream);
    if (c->scratch) (void)hipFree(c->scratch);
    c->scratch = nullptr; c->scratch_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 1 << 20);
    if (hipMalloc(&c->scratch, want) != hipSuccess) { g_last_error = "hipMalloc(scratch arena)"; return nullptr; }
    c->scratch_bytes = want;
    return c->scratch;
}
// Page-locked host arena of at least `bytes`, kept across calls (the host-pointer entry points are synchronous: nothing of an earlier call
// is in flight when the next one asks; growing drains the stream anyway).
void *orbhip_ctx_pinned_internal(orbhip_ctx *c, size_t bytes)
{
    if (bytes <= c->pinned_bytes) return c->pinned;
    (void)hipStreamSynchronize(c->stream);
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->pinned = nullptr; c->pinned_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 1 << 20);
    if (hipHostMalloc(&c->pinned, want, hipHostMallocDefault) != hipSuccess) { g_last_error = "hipHostMalloc(pinned staging arena)"; return nullptr; }
    c->pinned_bytes = want;
    return c->pinned;
}
// Cached device arena for one-shot BA solves (create + solve + download + destroy inside one call): nullptr when it is already lent
// out (the caller then allocates its own) or cannot be grown.
void *orbhip_ctx_ba_arena_acquire_internal(orbhip_ctx *c, size_t bytes)
{
    if (c->ba_arena_busy) return nullptr;
    if (bytes > c->ba_arena_bytes) {
        (void)hipStreamSynchronize(c->stream);
        if (c->ba_arena) (void)hipFree(c->ba_arena);
        c->ba_arena = nullptr; c->ba_arena_bytes = 0;
        const size_t want = bytes + bytes / 4;
        if (hipMalloc(&c->ba_arena, want) != hipSuccess) return nullptr;
        c->ba_arena_bytes = want;
    }
    c->ba_arena_busy = true;
    return c->ba_arena;
}
void orbhip_ctx_ba_arena_release_internal(orbhip_ctx *c) { c->ba_arena_busy = false; }
int *orbhip_ctx_pinned_word_internal(orbhip_ctx *c)
{
    if (!c->pinned_word && hipHostMalloc((void **)&c->pinned_word, 256, hipHostMallocDefault) != hipSuccess) c->pinned_word = nullptr;
    return c->pinned_word;
}
// Device work arena of at least `bytes`, kept across calls.  Growing waits for the stream (earlier kernels may still read the old arena).
void *orbhip_ctx_work_internal(orbhip_ctx *c, size_t bytes)
{
    if (bytes <= c->work_bytes) return c->work;
    (void)hipStreamSynchronize(c->stream);
    if (c->work) (void)hipFree(c->work);
    c->work = nullptr; c->work_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 20);
    if (hipMalloc(&c->work, want) != hipSuccess) { g_last_error = "hipMalloc(work arena)"; return nullptr; }
    c->work_bytes = want;
    return c->work;
}
void orbhip_set_last_error_internal(const char *msg) { g_last_error = msg; }
void orbhip_ctx_note_sbp_redo_internal(orbhip_ctx *c, size_t offset, int pairs) { c->sbp_redo_off = offset; c->sbp_redo_pairs = pairs; }
// Diagnostic: which pairs of the context's last SearchByProjection launch the replay form handed to the sequential kernel (include/orbhip.h)
extern "C" int orbhip_debug_sbp_handed_back(orbhip_ctx *c, int32_t *flags_out, int cap, int *pairs_out)
{
    if (!c || !pairs_out || cap < 0 || (cap > 0 && !flags_out)) return ORBHIP_E_BADARG;
    HIP_TRY(hipStreamSynchronize(c->stream));
    *pairs_out = c->sbp_redo_pairs;
    const int m = c->sbp_redo_pairs < cap ? c->sbp_redo_pairs : cap;
    if (m > 0) {
        if (!c->work || c->sbp_redo_off + sizeof(int32_t) * (size_t)m > c->work_bytes) return ORBHIP_E_BADARG;
        HIP_TRY(hipMemcpy(flags_out, (const uint8_t *)c->work + c->sbp_redo_off, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    }
    return ORBHIP_OK;
}
extern "C" int orbhip_ctx_check_status(orbhip_ctx *c)
{
    if (!c) return ORBHIP_E_BADARG;
    int32_t st = 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&st, orbhip_ctx_status_internal(c), sizeof(st), hipMemcpyDeviceToHost));
    if (st) { HIP_TRY(hipMemset(orbhip_ctx_status_internal(c), 0, sizeof(int32_t))); g_last_error = "device-side capacity exceeded in a matcher kernel"; }
    return st;
}
int32_t *orbhip_ctx_status_internal(orbhip_ctx *c) { return c->status_redirect ? c->status_redirect : c->d_status; }
// A host-pointer call (host_entry.hip) points the kernels' status word at a slot of its own blob for the duration of the call, so that the
// word travels with the call's single upload (zeroed) and single download instead of costing a copy of its own; nullptr restores
void orbhip_ctx_redirect_status_internal(orbhip_ctx *c, int32_t *p) { c->status_redirect = p; }
extern "C" void orbhip_ctx_destroy(orbhip_ctx *c)
{
    if (!c) return;
    (void)hipFree(c->d_status);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->work) (void)hipFree(c->work);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->ba_arena) (void)hipFree(c->ba_arena);
    if (c->pinned_word) (void)hipHostFree(c->pinned_word);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
extern "C" int orbhip_ctx_synchronize(orbhip_ctx *c)
{
    if (!c) return ORBHIP_E_BADARG;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}
// Stream order across two contexts of one device: everything submitted to `other` so far completes before anything submitted to `c`
// after this call starts.  What a caller needs to run, say, the two matchers of a frame pair side by side on two contexts and to keep the
// next extraction from overwriting the arrays they still read.  No host synchronisation.
extern "C" int orbhip_ctx_wait_for(orbhip_ctx *c, orbhip_ctx *other)
{
    if (!c || !other) return ORBHIP_E_BADARG;
    if (c == other || c->stream == other->stream) return ORBHIP_OK;
    if (c->device != other->device) { g_last_error = "orbhip_ctx_wait_for: contexts of two devices"; return ORBHIP_E_BADARG; }
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, other->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, ev, 0));
    HIP_TRY(hipEventDestroy(ev));
    return ORBHIP_OK;
}
extern "C" void *orbhip_ctx_stream(orbhip_ctx *c) { return c ? (void *)c->stream : nullptr; }
hipStream_t orbhip_ctx_stream_internal(orbhip_ctx *c) { return c->stream; }
int orbhip_ctx_device_internal(orbhip_ctx *c) { return c->device; }
int orbhip_ctx_cus_internal(orbhip_ctx *c) { return c->n_cus; }
int orbhip_ctx_ba_schur_mode_internal(orbhip_ctx *c) { return c->ba_schur_mode; }
extern "C" int orbhip_ctx_set_ba_schur_mode(orbhip_ctx *c, int mode)
{
    if (!c || mode < 0 || mode > 2) return ORBHIP_E_BADARG;
    c->ba_schur_mode = mode;
    return ORBHIP_OK;
}

// ------------------------------------------------------------------------------------
static inline int cv_round_f(float v) { return (int)lrintf(v); }   // round-half-even
static inline int cv_round_d(double v) { return (int)lrint(v); }
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

#define ORBHIP_PROF_SLOTS 32
struct orbhip_extractor {
    orbhip_ctx *ctx;
    int nfeatures, nlevels, ini_th, min_th;
    float scale_factor;
    float scale[ORB_MAX_LEVELS], inv_scale[ORB_MAX_LEVELS], sigma2[ORB_MAX_LEVELS], inv_sigma2[ORB_MAX_LEVELS];
    int per_level[ORB_MAX_LEVELS];
    int umax[ORB_HALF_PATCH + 1];
    int gauss_q8[7];
    // reserved geometry
    int width, height, max_batch;
    bool level0_owned;          // level-0 buffer allocated (host path / stride mismatch)
    OrbParams P;
    FastParams F;
    std::vector<void *> allocs;
    size_t bytes_reserved;
    int last_batch;
    bool profiling;
    hipEvent_t ev[ORBHIP_PROF_SLOTS][ORBHIP_STAGE_COUNT + 1];   // ring of per-call stage marks
    int ev_calls;               // extract calls recorded since the last stage_ms() query
    bool ev_created;
    float stage_ms[ORBHIP_STAGE_COUNT];
    uint8_t *d_level0;          // owned level-0 storage
    int32_t *d_stereo_sad;      // [max_batch][max_kp] scratch of orbhip_compute_stereo_matches_device (lazy)
    // graph mode (small batches are launch bound): the 19 launches of one extract call replayed as one hipGraph
    bool graph_mode, graph_valid;
    // k_blur (memory-wait bound) runs beside k_fast_cells / k_octree (issue / latency bound) on a second stream of the extractor
    hipStream_t aux; hipEvent_t ev_fork, ev_join, ev_pyr; bool aux_ok; int overlap;
    hipGraphExec_t graph_exec;
    int g_w, g_h, g_batch, g_lap0, g_lap1;
    size_t level0_frame_stride; int level0_pitch;
    // host-pointer path (ORBextractor::operator()): the four result arrays are slices of ONE device allocation (counts | mono | keypoints |
    // descriptors) with a page-locked mirror, so a call ends in one device-to-host copy; the input is gathered in a page-locked image
    uint8_t *d_outblob; size_t outblob_bytes, ob_kp, ob_desc;      // offsets of the keypoint / descriptor slices
    uint8_t *h_out; uint8_t *h_in; size_t h_in_bytes; int32_t *h_status;
    uint8_t *h_pyr; size_t h_pyr_bytes;                             // page-locked landing area of the lazy pyramid copy-out
    unsigned long long generation, view_generation;                 // extract calls so far; the call whose results h_out holds
    int oct_dmax_tab;                                               // table depth of k_octree_tab for this geometry (0: it cannot run), whichever form is selected
};

extern "C" int orbhip_extractor_create(orbhip_ctx *ctx, int nfeatures, float scale_factor, int nlevels,
                                       int ini_th, int min_th, orbhip_extractor **out)
{
    if (!ctx || !out || nlevels < 1 || nlevels > ORB_MAX_LEVELS || nfeatures < 1 || !(scale_factor > 1.0f) || scale_factor > 2.0f)
        return ORBHIP_E_BADARG;     // k_resize stages the footprint of a 64x32 tile in LDS: scale factors up to 2
    orbhip_extractor *e = new orbhip_extractor();
    e->ctx = ctx; e->nfeatures = nfeatures; e->nlevels = nlevels; e->ini_th = ini_th; e->min_th = min_th;
    e->scale_factor = scale_factor;
    e->width = e->height = e->max_batch = 0; e->bytes_reserved = 0; e->last_batch = 0;
    e->profiling = false; e->ev_created = false; e->ev_calls = 0; e->d_level0 = nullptr; e->level0_owned = false;
    e->d_stereo_sad = nullptr;
    e->graph_mode = false; e->graph_valid = false; e->graph_exec = nullptr;
    e->aux = nullptr; e->ev_fork = e->ev_join = e->ev_pyr = nullptr; e->aux_ok = false; e->overlap = 1;
    e->d_outblob = nullptr; e->outblob_bytes = e->ob_kp = e->ob_desc = 0; e->h_out = e->h_in = e->h_pyr = nullptr; e->h_in_bytes = e->h_pyr_bytes = 0; e->h_status = nullptr;
    e->generation = 0; e->view_generation = ~0ull;
    memset(&e->P, 0, sizeof(e->P));
    memset(e->stage_ms, 0, sizeof(e->stage_ms));
    // scale tables, ORBextractor.cc:413-429
    e->scale[0] = 1.0f; e->sigma2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) { e->scale[i] = e->scale[i - 1] * scale_factor; e->sigma2[i] = e->scale[i] * e->scale[i]; }
    for (int i = 0; i < nlevels; i++) { e->inv_scale[i] = 1.0f / e->scale[i]; e->inv_sigma2[i] = 1.0f / e->sigma2[i]; }
    // per-level quota, ORBextractor.cc:433-445
    float factor = 1.0f / scale_factor;
    float desired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) { e->per_level[l] = cv_round_f(desired); sum += e->per_level[l]; desired *= factor; }
    e->per_level[nlevels - 1] = std::max(nfeatures - sum, 0);
    // umax, ORBextractor.cc:453-468
    int v, v0, vmax = (int)floor(ORB_HALF_PATCH * sqrtf(2.f) / 2 + 1), vmin = (int)ceil(ORB_HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = ORB_HALF_PATCH * ORB_HALF_PATCH;
    for (v = 0; v <= vmax; ++v) e->umax[v] = cv_round_d(sqrt(hp2 - v * v));
    for (v = ORB_HALF_PATCH, v0 = 0; v >= vmin; --v) { while (e->umax[v0] == e->umax[v0 + 1]) ++v0; e->umax[v] = v0; ++v0; }
    // cv::getGaussianKernel(7, 2, CV_32F) -> q8
    {
        float cf[7]; double s = 0;
        for (int i = 0; i < 7; i++) { double x = i - 3.0; cf[i] = (float)exp(-0.5 / 4.0 * x * x); s += cf[i]; }
        s = 1. / s;
        for (int i = 0; i < 7; i++) { cf[i] = (float)(cf[i] * s); e->gauss_q8[i] = cv_round_f(cf[i] * 256.f); }
    }
    *out = e;
    return ORBHIP_OK;
}

static void ext_free_all(orbhip_extractor *e)
{
    for (void *p : e->allocs) (void)hipFree(p);
    e->allocs.clear();
    e->bytes_reserved = 0; e->width = e->height = e->max_batch = 0; e->d_level0 = nullptr; e->d_stereo_sad = nullptr;
    if (e->h_out) (void)hipHostFree(e->h_out);
    if (e->h_in) (void)hipHostFree(e->h_in);
    if (e->h_pyr) (void)hipHostFree(e->h_pyr);
    if (e->h_status) (void)hipHostFree(e->h_status);
    e->h_out = e->h_in = e->h_pyr = nullptr; e->h_status = nullptr; e->h_in_bytes = e->h_pyr_bytes = 0; e->d_outblob = nullptr; e->view_generation = ~0ull;
    if (e->graph_valid) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_valid = false; }
}
static void ext_free_aux(orbhip_extractor *e)
{
    if (!e->aux_ok) return;
    (void)hipStreamSynchronize(e->aux);
    (void)hipEventDestroy(e->ev_fork); (void)hipEventDestroy(e->ev_join); (void)hipEventDestroy(e->ev_pyr); (void)hipStreamDestroy(e->aux);
    e->aux_ok = false;
}

extern "C" void orbhip_extractor_destroy(orbhip_extractor *e)
{
    if (!e) return;
    (void)hipStreamSynchronize(e->ctx->stream);
    ext_free_aux(e);
    ext_free_all(e);
    if (e->ev_created) for (auto &slot : e->ev) for (auto &ev : slot) (void)hipEventDestroy(ev);
    delete e;
}

extern "C" int orbhip_extractor_levels(const orbhip_extractor *e) { return e ? e->nlevels : ORBHIP_E_BADARG; }
extern "C" int orbhip_extractor_table(const orbhip_extractor *e, int which, float *out)
{
    if (!e || !out || which < 0 || which > 3) return ORBHIP_E_BADARG;
    const float *t = which == 0 ? e->scale : which == 1 ? e->inv_scale : which == 2 ? e->sigma2 : e->inv_sigma2;
    memcpy(out, t, sizeof(float) * e->nlevels);
    return ORBHIP_OK;
}
extern "C" int orbhip_extractor_features_per_level(const orbhip_extractor *e, int *out)
{
    if (!e || !out) return ORBHIP_E_BADARG;
    memcpy(out, e->per_level, sizeof(int) * e->nlevels);
    return ORBHIP_OK;
}
extern "C" int orbhip_extractor_umax(const orbhip_extractor *e, int *out16)
{
    if (!e || !out16) return ORBHIP_E_BADARG;
    memcpy(out16, e->umax, sizeof(int) * 16);
    return ORBHIP_OK;
}
extern "C" int orbhip_extractor_max_keypoints(const orbhip_extractor *e) { return e ? e->P.max_kp : ORBHIP_E_BADARG; }

template <typename T>
static int dev_alloc(orbhip_extractor *e, T **p, size_t count)
{
    void *q = nullptr;
    size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    hipError_t err = hipMalloc(&q, bytes);
    if (err != hipSuccess) { g_last_error = std::string("hipMalloc: ") + hipGetErrorString(err); return ORBHIP_E_HIP; }
    e->allocs.push_back(q);
    e->bytes_reserved += bytes;
    *p = (T *)q;
    return ORBHIP_OK;
}

// cv::resize INTER_LINEAR coefficient tables, host float math as OpenCV's.
static void resize_tables(int sn, int dn, bool horizontal, std::vector<int16_t> &ofs, std::vector<int16_t> &coef)
{
    double scale = 1. / ((double)dn / sn);
    ofs.resize(dn); coef.resize(2 * dn);
    for (int d = 0; d < dn; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= s;
        if (horizontal) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= sn - 1) { f = 0; s = sn - 1; }
        }
        int c0 = cv_round_f((1.f - f) * 2048), c1 = cv_round_f(f * 2048);
        ofs[d] = (int16_t)std::min(std::max(s, -32768), 32767);
        coef[2 * d] = (int16_t)std::min(std::max(c0, -32768), 32767);
        coef[2 * d + 1] = (int16_t)std::min(std::max(c1, -32768), 32767);
    }
}

// Half-width of the disc the rBRIEF pattern can sample, per patch row |dy| = 0 .. 18 (k_orient_desc_tiled fetches no chunk outside it).  A
// pattern point of norm n lands, for every angle, within n of the centre before rounding, and rounds to row dy only where |v| >= |dy| - 0.5:
// there |u| <= sqrt(R^2 - (|dy| - 0.5)^2), rounded.  R = the largest norm (18.385): rows and columns +-19 are never sampled
// (tests/test_blur_tile_bounds.py sweeps the kernel's float32 expressions over the angles against this table).
extern "C" int orbhip_blur_half_widths(int *out19)
{
    if (!out19) return ORBHIP_E_BADARG;
    static const int8_t pat[1024] = {
#include "orb_pattern.inc"
    };
    double R2 = 0;
    for (int i = 0; i < 512; i++) R2 = std::max(R2, (double)pat[2 * i] * pat[2 * i] + (double)pat[2 * i + 1] * pat[2 * i + 1]);
    for (int d = 0; d < ORB_EDGE; d++) {
        const double t = std::max(d - 0.5, 0.0), q = R2 - t * t;
        out19[d] = q > 0 ? std::min((int)floor(sqrt(q) + 0.5), 18) : -64;
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_reserve(orbhip_extractor *e, int width, int height, int max_batch)
{
    if (!e || width <= 0 || height <= 0 || max_batch <= 0) return ORBHIP_E_BADARG;
    if (e->width == width && e->height == height && e->max_batch >= max_batch) return ORBHIP_OK;
    if (width > 4096 + 2 * ORB_MINB || height > 4096 + 2 * ORB_MINB) { g_last_error = "image larger than 12-bit key packing"; return ORBHIP_E_BADARG; }
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    ext_free_all(e);
    OrbParams &P = e->P;
    memset(&P, 0, sizeof(P));
    P.nlevels = e->nlevels; P.ini_th = e->ini_th; P.min_th = e->min_th;
    memcpy(P.umax, e->umax, sizeof(P.umax));
    memcpy(P.gauss_q8, e->gauss_q8, sizeof(P.gauss_q8));
    int cells = 0, keys = 0, kps = 0, max_cell_cap = 0;
    for (int l = 0; l < e->nlevels; l++) {
        OrbLevel &L = P.lv[l];
        // ComputePyramid sizes, ORBextractor.cc:1156-1157
        L.w = cv_round_f((float)width * e->inv_scale[l]);
        L.h = cv_round_f((float)height * e->inv_scale[l]);
        // cell grid, ORBextractor.cc:771-781
        if (!orb_plan_cell_grid(L)) { g_last_error = "pyramid level smaller than one FAST cell"; return ORBHIP_E_BADARG; }
        if (L.wcell + 6 > 64 || L.hcell + 6 > 64) { g_last_error = "FAST cell exceeds the 64x64 LDS tile"; return ORBHIP_E_BADARG; }
        max_cell_cap = std::max(max_cell_cap, ((L.wcell + 1) / 2) * ((L.hcell + 1) / 2));
        L.cell_base = cells; cells += L.ncols * L.nrows;
        L.quota = e->per_level[l];
        // DistributeOctTree roots, ORBextractor.cc:541-543
        const int maxx = L.w - ORB_MINB, maxy = L.h - ORB_MINB;
        L.n_ini = (int)roundf((float)(maxx - ORB_MINB) / (maxy - ORB_MINB));
        if (L.n_ini < 1) { g_last_error = "nIni == 0 (image taller than 2x its width): undefined in the reference"; return ORBHIP_E_BADARG; }
        L.hx = (float)(maxx - ORB_MINB) / L.n_ini;
        L.scale = e->scale[l];
        L.size = (float)(int)(31 * e->scale[l]);              // ORBextractor.cc:862
        L.kp_base = kps; L.kp_cap = align_up(std::max(L.quota + 8, 4 * L.n_ini + 4), 4); kps += L.kp_cap;   // multiple of 4: k_orient_desc
    }
    // cell list capacity: 3x3 strict-greater NMS admits at most one keypoint per 2x2 block
    for (int l = 0; l < e->nlevels; l++) {
        OrbLevel &L = P.lv[l];
        L.cell_cap = max_cell_cap;
        L.key_base = keys;
        // candidates per level: bounded by the same 2x2 argument over the whole detection area
        L.key_cap = std::min(L.ncols * L.nrows * max_cell_cap, ((L.w - 2 * ORB_MINB + 1) / 2 + L.ncols) * ((L.h - 2 * ORB_MINB + 1) / 2 + L.nrows));
        L.key_cap = std::min(L.key_cap, 0xFFFFF);
        keys += align_up(L.key_cap, 4);
    }
    P.cells_per_frame = cells; P.keys_per_frame = keys; P.kps_per_frame = kps; P.max_kp = align_up(kps, 8);
    // plans: each stage's file turns the geometry into its kernels' parameters and host tables (no HIP call); uploads follow the allocations
    std::vector<FcRecord> cell_tab;
    orb_plan_fast(P, e->F, cell_tab);
    P.rows_min_batch = getenv("ORBHIP_ROWS_MIN_BATCH") ? atoi(getenv("ORBHIP_ROWS_MIN_BATCH")) : 16;     // measured: 1 frame 122 us (tiles) vs 158 us (rows), 32 frames 252 vs 222 us
    std::vector<int8_t> bm_th, bm_tv;
    const bool bm_ok = orb_plan_blur(P, bm_th, bm_tv);
    P.cell_list_frame_stride = (size_t)cells * max_cell_cap;
    int rc;
    const size_t B = (size_t)max_batch;
    for (int l = 0; l < e->nlevels; l++) {
        OrbLevel &L = P.lv[l];
        L.img_pitch = align_up(L.w, 64); L.blur_pitch = L.img_pitch;
        L.img_frame_stride = (size_t)L.img_pitch * L.h;
        // the blurred level holds either layout (the blur kernel, and with it the layout, is chosen per call by the batch size): row-major at
        // blur_pitch, or tiles of 16 x 8 pixels = 128 bytes (orb_internal.h); level bases and frame strides are multiples of 128 bytes.  Bytes
        // of edge tiles beyond w or h are never written and never sampled
        L.blur_tiles_x = (L.w + 15) / 16;
        L.blur_frame_stride = align_up(std::max((size_t)L.blur_pitch * L.h, (size_t)L.blur_tiles_x * ((L.h + 7) / 8) * 128), (size_t)128);
        if ((rc = dev_alloc(e, &L.img, B * L.img_frame_stride + 64))) return rc;
        if ((rc = dev_alloc(e, &L.blur, B * L.blur_frame_stride + 64))) return rc;
        if (l > 0) {
            std::vector<int16_t> xo, xa, yo, yb;
            resize_tables(P.lv[l - 1].w, L.w, true, xo, xa);
            resize_tables(P.lv[l - 1].h, L.h, false, yo, yb);
            int16_t *dxo, *dxa, *dyo, *dyb;
            if ((rc = dev_alloc(e, &dxo, xo.size()))) return rc;
            if ((rc = dev_alloc(e, &dxa, xa.size()))) return rc;
            if ((rc = dev_alloc(e, &dyo, yo.size()))) return rc;
            if ((rc = dev_alloc(e, &dyb, yb.size()))) return rc;
            HIP_TRY(hipMemcpy(dxo, xo.data(), xo.size() * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dxa, xa.data(), xa.size() * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dyo, yo.data(), yo.size() * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dyb, yb.data(), yb.size() * 2, hipMemcpyHostToDevice));
            L.xofs = dxo; L.xalpha = dxa; L.yofs = dyo; L.ybeta = dyb;
            L.xchunk = nullptr; L.ytab = nullptr;
            std::vector<uint32_t> xc, yt;
            if (orb_plan_resize(P, l, xo, xa, yo, yb, xc, yt)) {           // k_resize_rows takes the level
                uint32_t *dxc, *dyt;
                if ((rc = dev_alloc(e, &dxc, xc.size()))) return rc;
                if ((rc = dev_alloc(e, &dyt, yt.size()))) return rc;
                HIP_TRY(hipMemcpy(dxc, xc.data(), xc.size() * 4, hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(dyt, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
                L.xchunk = dxc; L.ytab = dyt;
            }
        }
    }
    e->d_level0 = P.lv[0].img; e->level0_pitch = P.lv[0].img_pitch; e->level0_frame_stride = P.lv[0].img_frame_stride;
    if (bm_ok) {   // k_blur_mfma can take this geometry: its operand tables
        uint4 *dth, *dtv;
        if ((rc = dev_alloc(e, &dth, bm_th.size() / 16))) return rc;
        if ((rc = dev_alloc(e, &dtv, bm_tv.size() / 16))) return rc;
        HIP_TRY(hipMemcpy(dth, bm_th.data(), bm_th.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dtv, bm_tv.data(), bm_tv.size(), hipMemcpyHostToDevice));
        P.bm_th = dth; P.bm_tv = dtv;
    }
    {   // k_fast_cells' cell table
        FcRecord *dct;
        if ((rc = dev_alloc(e, &dct, cell_tab.size()))) return rc;
        HIP_TRY(hipMemcpy(dct, cell_tab.data(), cell_tab.size() * sizeof(FcRecord), hipMemcpyHostToDevice));
        e->F.cell_tab = dct;
    }
    P.desc_blocks_cap = getenv("ORBHIP_TUNE_DESC_BLOCKS") ? atoi(getenv("ORBHIP_TUNE_DESC_BLOCKS")) : 0;
    orbhip_blur_half_widths(P.blur_hw);       // k_orient_desc_tiled: which columns of a patch row the rBRIEF pattern can sample
    if ((rc = dev_alloc(e, &P.cell_count, B * cells))) return rc;
    if ((rc = dev_alloc(e, &P.cell_list, B * P.cell_list_frame_stride))) return rc;
    if ((rc = dev_alloc(e, &P.keys, B * keys))) return rc;
    if ((rc = dev_alloc(e, &P.node_of, B * keys))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_kp, B * kps))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_perm, B * kps))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_wkey, B * kps))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_angle, B * kps))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_desc, B * kps * 32))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_count, B * e->nlevels))) return rc;
    if ((rc = dev_alloc(e, &P.lvl_ncand, B * e->nlevels))) return rc;
    if ((rc = dev_alloc(e, &P.status, 1))) return rc;
    {   // results: one allocation, [count B][mono B] | keypoints [B][max_kp] | descriptors [B][max_kp][32], slices 256-byte aligned
        auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
        e->ob_kp = up(8 * B); e->ob_desc = e->ob_kp + up(sizeof(orbhip_keypoint) * B * P.max_kp);
        e->outblob_bytes = e->ob_desc + up((size_t)32 * B * P.max_kp);
        if ((rc = dev_alloc(e, &e->d_outblob, e->outblob_bytes))) return rc;
        P.out_count = reinterpret_cast<int32_t *>(e->d_outblob); P.out_mono = P.out_count + B;
        P.out_kp = reinterpret_cast<orbhip_keypoint *>(e->d_outblob + e->ob_kp); P.out_desc = e->d_outblob + e->ob_desc;
    }
    HIP_TRY(hipMemset(P.status, 0, sizeof(int32_t)));
    // the octree kernel keeps its node arrays in LDS: capacity = the largest node count any level can reach -- quota + 3 in the
    // subdivision loop, but the first pass splits every root unconditionally (up to 4 * nIni nodes; wide images, small budgets)
    P.oct_nc = orb_octree_nc(P);
    if (orb_octree_lds_bytes(P.oct_nc) > 150 * 1024) { g_last_error = "per-level quota (or nIni) too large for the LDS-resident octree"; return ORBHIP_E_BADARG; }
    for (int k = 0; k < 3; k++)
        if ((rc = orb_lds_optin(orb_octree_func(k), e->ctx->device, orb_octree_lds_bytes(P.oct_nc)))) return rc;
    // the table form (k_octree_tab, then k_octree_redo on the lists deeper than its tables) unless ORBHIP_OCTREE=iterative when the extractor
    // reserves: the same bytes either way (every tests/test_gpu_orb.py test with either form)
    e->oct_dmax_tab = orb_octree_dmax(P);
    P.oct_dmax = getenv("ORBHIP_OCTREE") && !strcmp(getenv("ORBHIP_OCTREE"), "iterative") ? 0 : e->oct_dmax_tab;
    if ((rc = orb_lds_optin(orb_fast_cells_func(e->F.small_cells), e->ctx->device, sizeof(uint32_t) * (size_t)e->F.wave_dw))) return rc;
    if (e->F.use_runs && (rc = orb_lds_optin(orb_fast_runs_func(orb_fast_runs_nld(e->F)), e->ctx->device, sizeof(uint32_t) * (size_t)e->F.run_dw))) return rc;
    e->width = width; e->height = height; e->max_batch = max_batch;
    return ORBHIP_OK;
}

int orb_stereo_max_kp();                                // stereo_kernels.hip: the keys of k_stereo_median live in LDS
int orb_stereo_lds_optin(int device, int max_kp);

// Frame::ComputeStereoMatches (reference src/Frame.cc:802-980) on the results of the latest extract call of a
// left and a right extractor (same geometry, same batch); frame f of `left` pairs with frame f of `right`.
extern "C" int orbhip_compute_stereo_matches_device(orbhip_extractor *left, orbhip_extractor *right, float mb, float mbf,
                                                    float *d_u_right, float *d_depth, int32_t *d_n_matches)
{
    if (!left || !right || !d_u_right || !d_depth || !(mb > 0) || !(mbf > 0)) return ORBHIP_E_BADARG;
    if (left->P.max_kp > orb_stereo_max_kp() || right->P.max_kp > orb_stereo_max_kp()) {
        g_last_error = "stereo: max_keypoints " + std::to_string(std::max(left->P.max_kp, right->P.max_kp)) + " exceeds " + std::to_string(orb_stereo_max_kp()) +
                       ", the keys the median filter can hold in 160 KB of LDS";
        return ORBHIP_E_BADARG;
    }
    if (!left->max_batch || !right->max_batch || left->last_batch <= 0 || left->last_batch != right->last_batch ||
        left->width != right->width || left->height != right->height || left->nlevels != right->nlevels ||
        left->scale_factor != right->scale_factor || left->P.max_kp != right->P.max_kp) {
        g_last_error = "stereo: extractors must share geometry, feature budget and batch, and have extracted";
        return ORBHIP_E_BADARG;
    }
    HIP_TRY(hipSetDevice(left->ctx->device));
    {
        const int rc = orb_stereo_lds_optin(left->ctx->device, left->P.max_kp);      // sets g_last_error
        if (rc) return rc;
    }
    if (!left->d_stereo_sad) {
        int rc = dev_alloc(left, &left->d_stereo_sad, (size_t)left->max_batch * left->P.max_kp);
        if (rc) return rc;
    }
    if (right->ctx->stream != left->ctx->stream) {          // the right extractor's kernels must have finished
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, right->ctx->stream));
        HIP_TRY(hipStreamWaitEvent(left->ctx->stream, ev, 0));
        HIP_TRY(hipEventDestroy(ev));
    }
    StereoArgs A;
    memset(&A, 0, sizeof(A));
    for (int l = 0; l < left->nlevels; l++) {
        const OrbLevel &a = left->P.lv[l], &b = right->P.lv[l];
        A.lv[l].imgL = a.img; A.lv[l].imgR = b.img; A.lv[l].fsL = a.img_frame_stride; A.lv[l].fsR = b.img_frame_stride;
        A.lv[l].pitchL = a.img_pitch; A.lv[l].pitchR = b.img_pitch; A.lv[l].wR = b.w;
        A.lv[l].scale = left->scale[l]; A.lv[l].inv_scale = left->inv_scale[l];
    }
    A.nlevels = left->nlevels; A.batch = left->last_batch; A.max_kp = left->P.max_kp; A.rows0 = left->height;
    A.kpL = left->P.out_kp; A.kpR = right->P.out_kp; A.descL = left->P.out_desc; A.descR = right->P.out_desc;
    A.nL = left->P.out_count; A.nR = right->P.out_count;
    A.mb = mb; A.mbf = mbf; A.u_right = d_u_right; A.depth = d_depth; A.sad = left->d_stereo_sad; A.n_kept = d_n_matches;
    orb_launch_stereo(A, left->ctx->stream);
    HIP_TRY(hipGetLastError());
    if (right->ctx->stream != left->ctx->stream) {
        // ... and the right extractor's NEXT extraction must not overwrite its pyramid / keypoints / descriptors while the stereo
        // kernels on the left stream still read them (write-after-read): its stream waits for them
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, left->ctx->stream));
        HIP_TRY(hipStreamWaitEvent(right->ctx->stream, ev, 0));
        HIP_TRY(hipEventDestroy(ev));
    }
    return ORBHIP_OK;
}

// Host-pointer form for ONE stereo frame: what Frame::ComputeStereoMatches() of host/Frame.cc calls after the two extractors have run
// (src/Frame.cc:109-130).  mvuRight / mvDepth of frame 0 of the latest extractions, n = its left keypoint count.
extern "C" int orbhip_compute_stereo_matches_host(orbhip_extractor *left, orbhip_extractor *right, float mb, float mbf,
                                                  float *u_right_out, float *depth_out, int n, int32_t *n_matches_out)
{
    if (!left || !right || n < 0 || (n && (!u_right_out || !depth_out))) return ORBHIP_E_BADARG;
    if (n_matches_out) *n_matches_out = 0;
    for (int i = 0; i < n; i++) { u_right_out[i] = -1.0f; depth_out[i] = -1.0f; }      // Frame.cc:804-805
    if (n == 0) return ORBHIP_OK;
    if (left->last_batch <= 0 || n > left->P.max_kp) { g_last_error = "stereo: the left extractor holds no extraction of that many keypoints"; return ORBHIP_E_BADARG; }
    const size_t slots = (size_t)left->max_batch * left->P.max_kp;
    uint8_t *w = (uint8_t *)orbhip_ctx_work_internal(left->ctx, 8 * slots + 4 * (size_t)left->max_batch + 256);
    if (!w) return ORBHIP_E_HIP;
    float *d_ur = (float *)w, *d_dp = d_ur + slots;
    int32_t *d_nk = (int32_t *)(d_dp + slots);
    const int rc = orbhip_compute_stereo_matches_device(left, right, mb, mbf, d_ur, d_dp, d_nk);
    if (rc) return rc;
    uint8_t *h = (uint8_t *)orbhip_ctx_pinned_internal(left->ctx, 8 * (size_t)n + 16);
    if (!h) return ORBHIP_E_HIP;
    hipStream_t st = left->ctx->stream;
    HIP_TRY(hipMemcpyAsync(h, d_ur, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h + 4 * (size_t)n, d_dp, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h + 8 * (size_t)n, d_nk, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(u_right_out, h, 4 * (size_t)n); memcpy(depth_out, h + 4 * (size_t)n, 4 * (size_t)n);
    if (n_matches_out) memcpy(n_matches_out, h + 8 * (size_t)n, 4);
    return ORBHIP_OK;
}

// Host-pointer form for ONE stereo-fisheye frame: what Frame::ComputeStereoFishEyeMatches() of host/Frame.cc calls after the two extractors
// have run with lapping {0, 511} (src/Frame.cc:1056-1097).  Frame 0 of both extractors' latest HOST extractions (n_left / n_right must be
// their counts); the outputs lie in one slice of the work arena and come back in one device-to-host copy.
extern "C" int orbhip_compute_stereo_fisheye_matches_host(orbhip_extractor *left, orbhip_extractor *right, int cam1_type, const float *cam1,
        int cam2_type, const float *cam2, const float *Rlr, const float *tlr, const float *level_sigma2, int nlevels,
        int32_t *l2r_out, float *depth_out, float *x3d_out, int n_left, int32_t *r2l_out, int n_right, int32_t *n_matches_out)
{
    if (!left || !right || n_left < 0 || n_right < 0 || (n_left && (!l2r_out || !depth_out || !x3d_out)) || (n_right && !r2l_out)) return ORBHIP_E_BADARG;
    if (n_matches_out) *n_matches_out = 0;
    for (int i = 0; i < n_left; i++) { l2r_out[i] = -1; depth_out[i] = -1.0f; x3d_out[3 * i] = x3d_out[3 * i + 1] = x3d_out[3 * i + 2] = 0.0f; }   // Frame.cc:1137-1141
    for (int i = 0; i < n_right; i++) r2l_out[i] = -1;
    if (n_left == 0) return ORBHIP_OK;
    const orbhip_keypoint *dk, *hk; const uint8_t *dd, *hd; int32_t cl = -1, cr = -1;
    if (orbhip_extractor_last_frame(left, 0, &dk, &dd, &hk, &hd, &cl, nullptr) != ORBHIP_OK || cl != n_left ||
        orbhip_extractor_last_frame(right, 0, &dk, &dd, &hk, &hd, &cr, nullptr) != ORBHIP_OK || cr != n_right) {
        g_last_error = "stereo fisheye: n_left / n_right are not the counts of the extractors' latest host extractions";
        return ORBHIP_E_BADARG;
    }
    if (left->ctx->device != right->ctx->device) { g_last_error = "stereo fisheye: extractors on two devices"; return ORBHIP_E_BADARG; }
    HIP_TRY(hipSetDevice(left->ctx->device));
    const int max_n = std::max(n_left, n_right);
    const size_t words = 6 * (size_t)max_n + 1;                     // l2r | r2l | depth | x3d [3] | n_matches
    int32_t *w = (int32_t *)orbhip_ctx_work_internal(left->ctx, 4 * words + 256);
    if (!w) return ORBHIP_E_HIP;
    int32_t *d_l2r = w, *d_r2l = w + max_n, *d_nm = w + 6 * (size_t)max_n;
    float *d_dp = (float *)(w + 2 * (size_t)max_n), *d_x = (float *)(w + 3 * (size_t)max_n);
    hipStream_t st = left->ctx->stream;
    if (right->ctx->stream != st) {                                 // the right extraction must have finished ...
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, right->ctx->stream));
        HIP_TRY(hipStreamWaitEvent(st, ev, 0));
        HIP_TRY(hipEventDestroy(ev));
    }
    const int rc = orbhip_compute_stereo_fisheye_matches_device(left->ctx, left->P.out_kp, left->P.out_desc, left->P.out_count, left->P.out_mono,
                                                                 left->P.max_kp, right->P.out_kp, right->P.out_desc, right->P.out_count,
                                                                 right->P.out_mono, right->P.max_kp, 1, max_n, cam1_type, cam1, cam2_type, cam2, Rlr,
                                                                 tlr, level_sigma2, nlevels, d_l2r, d_r2l, d_dp, d_x, d_nm);
    if (rc) return rc;
    if (right->ctx->stream != st) {                                 // ... and its next extraction must not overwrite what the kernels read
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, st));
        HIP_TRY(hipStreamWaitEvent(right->ctx->stream, ev, 0));
        HIP_TRY(hipEventDestroy(ev));
    }
    int32_t *h = (int32_t *)orbhip_ctx_pinned_internal(left->ctx, 4 * words + 16);
    if (!h) return ORBHIP_E_HIP;
    HIP_TRY(hipMemcpyAsync(h, w, 4 * words, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(l2r_out, h, 4 * (size_t)n_left);
    if (n_right) memcpy(r2l_out, h + max_n, 4 * (size_t)n_right);
    memcpy(depth_out, h + 2 * (size_t)max_n, 4 * (size_t)n_left);
    memcpy(x3d_out, h + 3 * (size_t)max_n, 12 * (size_t)n_left);
    if (n_matches_out) *n_matches_out = h[6 * (size_t)max_n];
    return ORBHIP_OK;
}

// which kernel blurs a batch of that many frames: 0 = the LDS tile kernel, 1 = k_blur_rows, 2 = k_blur_mfma (bench.py labels its stage with it)
extern "C" int orbhip_extractor_blur_kernel(const orbhip_extractor *e, int batch)
{
    if (!e || !e->max_batch) return -1;
    return orb_blur_kernel(e->P, batch);
}

// which instance runs the per-cell FAST stage on this extractor's geometry: 0 = k_fast_cells<5, 32, 5> (large cells), 1 = k_fast_cells<3, 24, 2>
// (small cells), 2 = k_fast_runs<4>, 3 = k_fast_runs<6> (ORBHIP_FAST_KERNEL=runs when the extractor reserved); orb_launch_fast_cells' own choice
extern "C" int orbhip_extractor_fast_kernel(const orbhip_extractor *e)
{
    if (!e || !e->max_batch) return -1;
    return orb_fast_variant(e->F);
}

// layout of the blurred pyramid after a call with that many frames: 1 = tiles of 16 x 8 pixels (the matrix-core blur writes them unless
// ORBHIP_BLUR_TILED=0 was set when the extractor reserved), 0 = row-major.  orbhip_extractor_get_blurred_level de-tiles either way.
extern "C" int orbhip_extractor_blur_tiled(const orbhip_extractor *e, int batch)
{
    if (!e || !e->max_batch) return -1;
    return e->P.blur_tiled_ok && orb_blur_kernel(e->P, batch) == 2 ? 1 : 0;
}

// output rows per band of k_resize_rows at that level (tests pick geometries by it); 0 = the level has no row tables (k_resize)
extern "C" int orbhip_extractor_resize_band_rows(const orbhip_extractor *e, int level)
{
    if (!e || !e->max_batch || level < 1 || level >= e->nlevels) return -1;
    return e->P.lv[level].xchunk ? e->P.lv[level].rs_rows : 0;
}

extern "C" int orbhip_extractor_set_profiling(orbhip_extractor *e, int enable)
{
    if (!e) return ORBHIP_E_BADARG;
    if (enable && !e->ev_created) {
        for (auto &slot : e->ev) for (auto &ev : slot) HIP_TRY(hipEventCreate(&ev));
        e->ev_created = true;
    }
    e->profiling = enable != 0;
    e->ev_calls = 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_stage_ms(orbhip_extractor *e, float *ms_out)
{
    if (!e || !ms_out || !e->ev_created || e->ev_calls <= 0) return ORBHIP_E_BADARG;
    // average over the (up to ORBHIP_PROF_SLOTS) most recent extract calls since the last query
    const int n = std::min(e->ev_calls, ORBHIP_PROF_SLOTS);
    for (int i = 0; i < ORBHIP_STAGE_COUNT; i++) ms_out[i] = 0.f;
    for (int c = 0; c < n; c++) {
        const int slot = (e->ev_calls - 1 - c) % ORBHIP_PROF_SLOTS;
        HIP_TRY(hipEventSynchronize(e->ev[slot][ORBHIP_STAGE_COUNT]));
        for (int i = 0; i < ORBHIP_STAGE_COUNT; i++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, e->ev[slot][i], e->ev[slot][i + 1]));
            ms_out[i] += ms / n;
        }
    }
    e->ev_calls = 0;
    return ORBHIP_OK;
}

static int tune_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }      // tuning hook (development)

static int run_pipeline(orbhip_extractor *e, int batch, int lap0, int lap1)
{
    OrbParams &P = e->P;
    P.batch = batch; P.lap0 = lap0; P.lap1 = lap1; P.n_cus = e->ctx->n_cus;
    P.blur_tiled = orbhip_extractor_blur_tiled(e, batch) == 1;       // exactly when orb_launch_blur takes k_blur_mfma
    hipStream_t s = e->ctx->stream;
    const bool prof = e->profiling;
    const int slot = e->ev_calls % ORBHIP_PROF_SLOTS;
#define STAGE_MARK(i) do { if (prof) HIP_TRY(hipEventRecord(e->ev[slot][i], s)); } while (0)
#define FAST_TRY(launch) do { if (!(launch)) { g_last_error = "batch * FAST cells exceeds the 32-bit cell counter of k_fast_cells"; return ORBHIP_E_BADARG; } } while (0)
    // fork: two streams inside one call.  Stage profiling measures the kernels one by one on one stream.
    const bool fork = e->overlap && !prof && batch >= ORB_OVERLAP_MIN_BATCH;
    if (fork && !e->aux_ok) {
        HIP_TRY(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_pyr, hipEventDisableTiming));
        e->aux_ok = true;
    }
    FastParams &F = e->F;
    for (int l = 0; l < e->nlevels; l++) { F.im[l].img = P.lv[l].img; F.im[l].frame_stride = P.lv[l].img_frame_stride; F.im[l].pitch = P.lv[l].img_pitch; }
    F.batch = batch; F.n_cus = e->ctx->n_cus; F.cell_count = P.cell_count; F.cell_list = P.cell_list; F.cell_list_frame_stride = P.cell_list_frame_stride; F.status = P.status;
    const bool rows = orb_blur_kernel(P, batch) != 0;               // the row-streaming / matrix-core blur needs no LDS: k_fast_cells keeps its full grid
    // waves of k_fast_cells per CU while the blur runs beside it: 10 next to the LDS tile blur; 18 (of the 23 the LDS would hold) next to the
    // row-streaming / matrix-core kernels, which need wave slots and registers, not LDS -- measured in one call on one box (round 4, 1024 VGA
    // frames, matrix-core blur): 23 waves 3.79 ms per step, 22: 3.84, 20: 3.72, 18: 3.69, 16: 3.74, 14: 3.80; 1080p / 512 frames
    // (row-streaming blur): 49.2 k -> 50.7 k frames/s; VGA with the row-streaming blur: 3.82 either way
    const int fast_waves = fork ? tune_int("ORBHIP_TUNE_FAST_WAVES", rows ? 18 : 10) : 0;
    STAGE_MARK(ORBHIP_STAGE_PYRAMID);
    if (fork && e->nlevels > 1 && rows && tune_int("ORBHIP_TUNE_L0_EARLY", 0)) {
        // (off by default: measured 3.90 ms vs 3.84 ms per step)
        // Level 0 is the input itself: its FAST cells (a third of all pixels) start at once on the main stream, the pyramid is built
        // beside them on the second stream (k_resize_rows needs a few KB of LDS, k_fast_cells leaves half of the wave slots free and
        // ~40 % of the issue cycles idle); levels 1.. follow when the pyramid is there, the blur runs beside them.
        HIP_TRY(hipEventRecord(e->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        FAST_TRY(orb_launch_fast_cells(F, s, fast_waves, 0, 1));
        for (int l = 1; l < e->nlevels; l++) orb_launch_resize(P, l, e->aux);
        HIP_TRY(hipEventRecord(e->ev_pyr, e->aux));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_pyr, 0));
        FAST_TRY(orb_launch_fast_cells(F, s, fast_waves, 1, e->nlevels));
        orb_launch_blur(P, e->aux, 5);
        HIP_TRY(hipEventRecord(e->ev_join, e->aux));
    } else {
        for (int l = 1; l < e->nlevels; l++) orb_launch_resize(P, l, s);
        STAGE_MARK(ORBHIP_STAGE_FAST_CELLS);
        if (fork) {                                         // the blur only needs the pyramid; it joins before the descriptors
            HIP_TRY(hipEventRecord(e->ev_fork, s));
            HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        }
        FAST_TRY(orb_launch_fast_cells(F, s, fast_waves));
        if (fork) {                                         // after k_fast_cells on purpose: its waves take their LDS first, the blur fills the free wave slots
            if (!tune_int("ORBHIP_TUNE_SKIP_BLUR", 0))       // (timing experiment only: descriptors are wrong without the blur)
                orb_launch_blur(P, e->aux, tune_int("ORBHIP_TUNE_BLUR_WGS", 5));
            HIP_TRY(hipEventRecord(e->ev_join, e->aux));
        }
    }
    STAGE_MARK(ORBHIP_STAGE_BLUR);
    if (!fork) orb_launch_blur(P, s, 8);
    STAGE_MARK(ORBHIP_STAGE_OCTREE);
    orb_launch_octree(P, s);
    STAGE_MARK(ORBHIP_STAGE_DESC);
    if (fork) HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
    orb_launch_orient_desc(P, s);
    STAGE_MARK(ORBHIP_STAGE_ASSEMBLE);
    orb_launch_assemble(P, s);
    STAGE_MARK(ORBHIP_STAGE_COUNT);
#undef STAGE_MARK
#undef FAST_TRY
    if (prof) e->ev_calls++;
    HIP_TRY(hipGetLastError());
    e->last_batch = batch;
    e->generation++;
    return ORBHIP_OK;
}

// Graph mode: capture the launches of run_pipeline once per (size, batch, lapping), then replay.  The caller has
// staged the input into the extractor's own level-0 buffer (fixed addresses).
static int run_pipeline_graph(orbhip_extractor *e, int width, int height, int batch, int lap0, int lap1)
{
    if (!(e->graph_valid && e->g_w == width && e->g_h == height && e->g_batch == batch && e->g_lap0 == lap0 && e->g_lap1 == lap1)) {
        if (e->graph_valid) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_valid = false; }
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(e->ctx->stream, hipStreamCaptureModeThreadLocal));
        const int rc = run_pipeline(e, batch, lap0, lap1);
        hipError_t ce = hipStreamEndCapture(e->ctx->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ce != hipSuccess) { g_last_error = std::string("hipStreamEndCapture: ") + hipGetErrorString(ce); return ORBHIP_E_HIP; }
        hipError_t ie = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) { g_last_error = std::string("hipGraphInstantiate: ") + hipGetErrorString(ie); return ORBHIP_E_HIP; }
        e->graph_valid = true; e->g_w = width; e->g_h = height; e->g_batch = batch; e->g_lap0 = lap0; e->g_lap1 = lap1;
    }
    HIP_TRY(hipGraphLaunch(e->graph_exec, e->ctx->stream));
    e->last_batch = batch;
    e->generation++;
    return ORBHIP_OK;
}

extern "C" int orbhip_extract_batch_device(orbhip_extractor *e, const uint8_t *d_images, int width, int height,
                                           size_t row_stride, size_t frame_stride, int batch, int lap0, int lap1)
{
    if (!e || batch <= 0 || row_stride < (size_t)width) return ORBHIP_E_BADARG;
    if (!d_images || width <= 0 || height <= 0) return ORBHIP_E_EMPTY;
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = orbhip_extractor_reserve(e, width, height, batch);
    if (rc) return rc;
    // level 0 of the pyramid is the input itself (the reference copies it into a padded
    // buffer, ORBextractor.cc:1172; the bytes are identical): alias, do not copy -- unless the caller's
    // layout would break the kernels' aligned dword row accesses, then stage it once on the device.
    OrbLevel &L0 = e->P.lv[0];
    const bool aligned = ((uintptr_t)d_images % 4 == 0) && (row_stride % 4 == 0) && (frame_stride % 4 == 0);
    const bool use_graph = e->graph_mode && !e->profiling;
    if (aligned && !use_graph) {
        L0.img = const_cast<uint8_t *>(d_images);
        L0.img_pitch = (int)row_stride;
        L0.img_frame_stride = frame_stride;
    } else {                    // graph mode always stages: the captured kernels must see fixed addresses
        L0.img = e->d_level0; L0.img_pitch = e->level0_pitch; L0.img_frame_stride = e->level0_frame_stride;
        for (int f = 0; f < batch; f++)
            HIP_TRY(hipMemcpy2DAsync(L0.img + (size_t)f * L0.img_frame_stride, L0.img_pitch, d_images + (size_t)f * frame_stride,
                                     row_stride, width, height, hipMemcpyDeviceToDevice, e->ctx->stream));
    }
    return use_graph ? run_pipeline_graph(e, width, height, batch, lap0, lap1) : run_pipeline(e, batch, lap0, lap1);
}

// Small batches are launch bound (19 kernels per extract call): with graph mode on, the launches of one call are
// captured once per (size, batch, lapping) and replayed as a single hipGraph; the input is then always staged into
// the extractor's own level-0 buffer (one D2D copy) so that the captured kernels see fixed addresses.
extern "C" int orbhip_extractor_set_graph_mode(orbhip_extractor *e, int enable)
{
    if (!e) return ORBHIP_E_BADARG;
    e->graph_mode = enable != 0;
    if (!e->graph_mode && e->graph_valid) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_valid = false; }
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_results(orbhip_extractor *e, orbhip_keypoint **d_kp, uint8_t **d_desc,
                                        int32_t **d_count, int32_t **d_mono)
{
    if (!e || !e->max_batch) return ORBHIP_E_BADARG;
    if (d_kp) *d_kp = e->P.out_kp;
    if (d_desc) *d_desc = e->P.out_desc;
    if (d_count) *d_count = e->P.out_count;
    if (d_mono) *d_mono = e->P.out_mono;
    return ORBHIP_OK;
}

// Host-pointer extraction (what ORBextractor::operator() is): the image rows are gathered into a page-locked copy laid out like the
// device's level 0 and leave in ONE host-to-device copy; the results (counts, mono indices, keypoints, descriptors -- one device
// allocation) come back in ONE device-to-host copy into their page-locked mirror, the status word beside them, one synchronisation.
// round 3 issued one pageable 2-D copy per frame in, two synchronisations and 2 + 2 per-frame copies out.
static int extract_host_core(orbhip_extractor *e, const uint8_t *h_images, int width, int height, size_t row_stride, size_t frame_stride,
                             int batch, int lap0, int lap1)
{
    if (!e || batch <= 0) return ORBHIP_E_BADARG;
    if (!h_images || width <= 0 || height <= 0) return ORBHIP_E_EMPTY;      // ORBextractor.cc:1072-1073
    if (row_stride < (size_t)width) return ORBHIP_E_BADARG;
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = orbhip_extractor_reserve(e, width, height, batch);
    if (rc) return rc;
    hipStream_t s = e->ctx->stream;
    OrbLevel &L0 = e->P.lv[0];
    L0.img = e->d_level0; L0.img_pitch = e->level0_pitch; L0.img_frame_stride = e->level0_frame_stride;
    const size_t in_bytes = (size_t)batch * L0.img_frame_stride;
    if (e->h_in_bytes < in_bytes) {
        if (e->h_in) (void)hipHostFree(e->h_in);
        e->h_in = nullptr; e->h_in_bytes = 0;
        HIP_TRY(hipHostMalloc((void **)&e->h_in, (size_t)e->max_batch * L0.img_frame_stride, hipHostMallocDefault));
        e->h_in_bytes = (size_t)e->max_batch * L0.img_frame_stride;
    }
    if (!e->h_out) HIP_TRY(hipHostMalloc((void **)&e->h_out, e->outblob_bytes, hipHostMallocDefault));
    if (!e->h_status) HIP_TRY(hipHostMalloc((void **)&e->h_status, 256, hipHostMallocDefault));
    for (int f = 0; f < batch; f++) {
        const uint8_t *src = h_images + (size_t)f * frame_stride;
        uint8_t *dst = e->h_in + (size_t)f * L0.img_frame_stride;
        if (row_stride == (size_t)L0.img_pitch) memcpy(dst, src, (size_t)L0.img_pitch * (height - 1) + width);
        else for (int y = 0; y < height; y++) memcpy(dst + (size_t)y * L0.img_pitch, src + (size_t)y * row_stride, width);
    }
    HIP_TRY(hipMemcpyAsync(L0.img, e->h_in, in_bytes, hipMemcpyHostToDevice, s));
    e->view_generation = ~0ull;
    rc = (e->graph_mode && !e->profiling) ? run_pipeline_graph(e, width, height, batch, lap0, lap1) : run_pipeline(e, batch, lap0, lap1);
    if (rc) return rc;
    const size_t B = (size_t)e->max_batch, mk = (size_t)e->P.max_kp;
    if ((size_t)batch == B) HIP_TRY(hipMemcpyAsync(e->h_out, e->d_outblob, e->outblob_bytes, hipMemcpyDeviceToHost, s));
    else {                                                                   // a smaller batch than reserved: the used rows of each slice
        HIP_TRY(hipMemcpyAsync(e->h_out, e->d_outblob, 8 * B, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(e->h_out + e->ob_kp, e->d_outblob + e->ob_kp, sizeof(orbhip_keypoint) * mk * batch, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(e->h_out + e->ob_desc, e->d_outblob + e->ob_desc, 32 * mk * batch, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(e->h_status, e->P.status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*e->h_status) {
        g_last_error = "device-side list capacity exceeded";
        (void)hipMemsetAsync(e->P.status, 0, sizeof(int32_t), s);
        return *e->h_status;
    }
    e->view_generation = e->generation;
    return ORBHIP_OK;
}

extern "C" int orbhip_extract_batch_host(orbhip_extractor *e, const uint8_t *h_images, int width, int height,
                                         size_t row_stride, size_t frame_stride, int batch, int lap0, int lap1,
                                         orbhip_keypoint *kp_out, uint8_t *desc_out, int cap,
                                         int32_t *count_out, int32_t *mono_out)
{
    if (e && batch > 0 && h_images && width > 0 && height > 0 && (!kp_out || !desc_out || !count_out || !mono_out)) return ORBHIP_E_BADARG;
    const int rc = extract_host_core(e, h_images, width, height, row_stride, frame_stride, batch, lap0, lap1);
    if (rc) return rc;
    const int32_t *cnt = reinterpret_cast<const int32_t *>(e->h_out), *mono = cnt + e->max_batch;
    const size_t mk = (size_t)e->P.max_kp;
    for (int f = 0; f < batch; f++) {
        count_out[f] = cnt[f]; mono_out[f] = mono[f];
        if (cnt[f] > cap) return ORBHIP_E_CAPACITY;
        if (cnt[f] == 0) continue;
        memcpy(kp_out + (size_t)f * cap, e->h_out + e->ob_kp + sizeof(orbhip_keypoint) * mk * f, sizeof(orbhip_keypoint) * cnt[f]);
        memcpy(desc_out + (size_t)f * cap * 32, e->h_out + e->ob_desc + 32 * mk * f, (size_t)32 * cnt[f]);
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_extract_batch_host_view(orbhip_extractor *e, const uint8_t *h_images, int width, int height, size_t row_stride,
                                              size_t frame_stride, int batch, int lap0, int lap1, const orbhip_keypoint **kp_view,
                                              const uint8_t **desc_view, int *row_capacity, const int32_t **count_view, const int32_t **mono_view)
{
    if (e && batch > 0 && h_images && width > 0 && height > 0 && (!kp_view || !desc_view || !row_capacity || !count_view || !mono_view)) return ORBHIP_E_BADARG;
    const int rc = extract_host_core(e, h_images, width, height, row_stride, frame_stride, batch, lap0, lap1);
    if (rc) return rc;
    *kp_view = reinterpret_cast<const orbhip_keypoint *>(e->h_out + e->ob_kp); *desc_view = e->h_out + e->ob_desc; *row_capacity = e->P.max_kp;
    *count_view = reinterpret_cast<const int32_t *>(e->h_out); *mono_view = *count_view + e->max_batch;
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_last_frame(orbhip_extractor *e, int frame, const orbhip_keypoint **d_kp, const uint8_t **d_desc,
                                           const orbhip_keypoint **h_kp_view, const uint8_t **h_desc_view, int32_t *count, unsigned long long *generation)
{
    if (!e || !e->max_batch || frame < 0 || frame >= e->last_batch || e->view_generation != e->generation) return ORBHIP_E_BADARG;
    const size_t mk = (size_t)e->P.max_kp;
    if (d_kp) *d_kp = e->P.out_kp + mk * frame;
    if (d_desc) *d_desc = e->P.out_desc + 32 * mk * frame;
    if (h_kp_view) *h_kp_view = reinterpret_cast<const orbhip_keypoint *>(e->h_out + e->ob_kp) + mk * frame;
    if (h_desc_view) *h_desc_view = e->h_out + e->ob_desc + 32 * mk * frame;
    if (count) *count = reinterpret_cast<const int32_t *>(e->h_out)[frame];
    if (generation) *generation = e->generation;
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_desc_plan(const orbhip_extractor *e, int batch, int32_t *kp_base, int32_t *kp_cap, int32_t *waves_per_xcd)
{
    if (!e || !e->max_batch || batch < 1 || batch > e->max_batch) return ORBHIP_E_BADARG;
    for (int l = 0; l < e->nlevels; l++) { kp_base[l] = e->P.lv[l].kp_base; kp_cap[l] = e->P.lv[l].kp_cap; }
    OrbParams P = e->P;
    P.batch = batch;
    *waves_per_xcd = 2 * orb_orient_desc_blocks(P);
    return ORBHIP_OK;
}

// ------------------------------------------------------------------------------------ taps
extern "C" int orbhip_extractor_level_dims(const orbhip_extractor *e, int level, int *w, int *h)
{
    if (!e || level < 0 || level >= e->nlevels || !e->max_batch) return ORBHIP_E_BADARG;
    *w = e->P.lv[level].w; *h = e->P.lv[level].h;
    return ORBHIP_OK;
}

static inline int reflect101_host(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
    return p;
}

extern "C" int orbhip_extractor_get_pyramid_level(orbhip_extractor *e, int frame, int level, int padded,
                                                  uint8_t *h_out, size_t out_stride)
{
    if (!e || !h_out || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch) return ORBHIP_E_BADARG;
    const OrbLevel &L = e->P.lv[level];
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    if (!padded) {
        HIP_TRY(hipMemcpy2D(h_out, out_stride, L.img + (size_t)frame * L.img_frame_stride, L.img_pitch, L.w, L.h, hipMemcpyDeviceToHost));
        return ORBHIP_OK;
    }
    // mvImagePyramid's parent buffer: ROI + 19-px BORDER_REFLECT_101 (ORBextractor.cc:1167,1172),
    // synthesised lazily on copy-out; the extraction itself never reads the border.
    std::vector<uint8_t> tmp((size_t)L.w * L.h);
    HIP_TRY(hipMemcpy2D(tmp.data(), L.w, L.img + (size_t)frame * L.img_frame_stride, L.img_pitch, L.w, L.h, hipMemcpyDeviceToHost));
    const int pw = L.w + 2 * ORB_EDGE, ph = L.h + 2 * ORB_EDGE;
    for (int y = 0; y < ph; y++) {
        const uint8_t *srow = tmp.data() + (size_t)reflect101_host(y - ORB_EDGE, L.h) * L.w;
        uint8_t *drow = h_out + (size_t)y * out_stride;
        for (int x = 0; x < pw; x++) drow[x] = srow[reflect101_host(x - ORB_EDGE, L.w)];
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_get_pyramid_padded(orbhip_extractor *e, int frame, uint8_t *const *levels_out, const size_t *strides)
{
    if (!e || !levels_out || !strides || frame < 0 || frame >= e->last_batch) return ORBHIP_E_BADARG;
    HIP_TRY(hipSetDevice(e->ctx->device));
    hipStream_t s = e->ctx->stream;
    // every level is one linear device-to-host copy (pitch x rows, page-locked landing area); rows are then laid into the caller's
    // padded parents on the host, where the border has to be synthesised anyway
    size_t total = 0;
    for (int l = 0; l < e->nlevels; l++) {
        const OrbLevel &L = e->P.lv[l];
        if (!levels_out[l] || strides[l] < (size_t)L.w + 2 * ORB_EDGE) return ORBHIP_E_BADARG;
        total += ((size_t)L.img_pitch * L.h + 255) & ~(size_t)255;
    }
    if (e->h_pyr_bytes < total) {
        if (e->h_pyr) (void)hipHostFree(e->h_pyr);
        e->h_pyr = nullptr; e->h_pyr_bytes = 0;
        HIP_TRY(hipHostMalloc((void **)&e->h_pyr, total, hipHostMallocDefault));
        e->h_pyr_bytes = total;
    }
    size_t off = 0;
    for (int l = 0; l < e->nlevels; l++) {
        const OrbLevel &L = e->P.lv[l];
        HIP_TRY(hipMemcpyAsync(e->h_pyr + off, L.img + (size_t)frame * L.img_frame_stride, (size_t)L.img_pitch * (L.h - 1) + L.w, hipMemcpyDeviceToHost, s));
        off += ((size_t)L.img_pitch * L.h + 255) & ~(size_t)255;
    }
    HIP_TRY(hipStreamSynchronize(s));
    off = 0;
    for (int l = 0; l < e->nlevels; l++) {
        const OrbLevel &L = e->P.lv[l];
        for (int y = 0; y < L.h; y++) memcpy(levels_out[l] + (size_t)(y + ORB_EDGE) * strides[l] + ORB_EDGE, e->h_pyr + off + (size_t)y * L.img_pitch, L.w);
        off += ((size_t)L.img_pitch * L.h + 255) & ~(size_t)255;
    }
    // the 19-px BORDER_REFLECT_101 frame (ORBextractor.cc:1167-1173), synthesised on the host: the extraction never reads it
    for (int l = 0; l < e->nlevels; l++) {
        const OrbLevel &L = e->P.lv[l];
        const size_t st = strides[l];
        uint8_t *base = levels_out[l];
        for (int y = ORB_EDGE; y < L.h + ORB_EDGE; y++) {
            uint8_t *row = base + (size_t)y * st;
            for (int x = 0; x < ORB_EDGE; x++) {
                row[x] = row[ORB_EDGE + reflect101_host(x - ORB_EDGE, L.w)];
                row[L.w + ORB_EDGE + x] = row[ORB_EDGE + reflect101_host(L.w + x, L.w)];
            }
        }
        for (int y = 0; y < ORB_EDGE; y++) {
            memcpy(base + (size_t)y * st, base + (size_t)(ORB_EDGE + reflect101_host(y - ORB_EDGE, L.h)) * st, (size_t)L.w + 2 * ORB_EDGE);
            memcpy(base + (size_t)(L.h + ORB_EDGE + y) * st, base + (size_t)(ORB_EDGE + reflect101_host(L.h + y, L.h)) * st, (size_t)L.w + 2 * ORB_EDGE);
        }
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_get_blurred_level(orbhip_extractor *e, int frame, int level, uint8_t *h_out, size_t out_stride)
{
    if (!e || !h_out || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch) return ORBHIP_E_BADARG;
    const OrbLevel &L = e->P.lv[level];
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    if (orbhip_extractor_blur_tiled(e, e->last_batch) == 1) {      // the last call wrote tiles: callers see the same row-major bytes
        const int tiles_x = L.blur_tiles_x, tiles_y = (L.h + 7) / 8;
        std::vector<uint8_t> t((size_t)tiles_x * tiles_y * 128);
        HIP_TRY(hipMemcpy(t.data(), L.blur + (size_t)frame * L.blur_frame_stride, t.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < L.h; y++)
            for (int x = 0; x < L.w; x += 16)
                memcpy(h_out + (size_t)y * out_stride + x, t.data() + ORB_BLUR_TILE_OFF(x, y, tiles_x), (size_t)std::min(16, L.w - x));
        return ORBHIP_OK;
    }
    HIP_TRY(hipMemcpy2D(h_out, out_stride, L.blur + (size_t)frame * L.blur_frame_stride, L.blur_pitch, L.w, L.h, hipMemcpyDeviceToHost));
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_get_fast_candidates(orbhip_extractor *e, int frame, int level, int32_t *xs, int32_t *ys,
                                                    int32_t *scores, int cap, int32_t *n_out)
{
    if (!e || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch || !n_out) return ORBHIP_E_BADARG;
    const OrbParams &P = e->P;
    const OrbLevel &L = P.lv[level];
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, P.lvl_ncand + frame * P.nlevels + level, sizeof(n), hipMemcpyDeviceToHost));
    *n_out = n;
    int m = std::min(n, cap);
    if (m > 0 && xs && ys && scores) {
        std::vector<uint32_t> k(m);
        HIP_TRY(hipMemcpy(k.data(), P.keys + (size_t)frame * P.keys_per_frame + L.key_base, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) { xs[i] = ORB_KEY_X(k[i]); ys[i] = ORB_KEY_Y(k[i]); scores[i] = ORB_KEY_S(k[i]); }
    }
    return ORBHIP_OK;
}

// Test entry: the octree stage alone, on candidate lists the caller supplies for ONE level of `nframes` frames (frame f owns entries
// offs[f] .. offs[f + 1] of xs / ys / scores; coordinates relative to the detection area, as the FAST stage produces them).  Each list is sorted
// into the level's FAST cells, row-major and stable, which is the list order the kernels see.  form 0 = iterative, 1 = table form (with its
// second launch).  out_keys[f * cap + i] = x | y << 12 | score << 24 of the i-th kept key, out_counts[f] their number, out_redo[f] (optional) = 1
// where the table form handed the list to the iterative form.
extern "C" int orbhip_debug_octree(orbhip_extractor *e, int level, int nframes, const int32_t *offs, const int32_t *xs, const int32_t *ys,
                                   const int32_t *scores, int form, uint32_t *out_keys, int cap, int32_t *out_counts, int32_t *out_redo)
{
    if (!e || !e->max_batch || level < 0 || level >= e->nlevels || nframes < 1 || nframes > e->max_batch || !offs || !out_keys || !out_counts ||
        form < 0 || form > 1 || cap < 0) return ORBHIP_E_BADARG;
    if (form == 1 && e->oct_dmax_tab <= 0) { g_last_error = "the table form of the octree cannot run at this geometry"; return ORBHIP_E_BADARG; }
    OrbParams P = e->P;
    const OrbLevel &L = P.lv[level];
    P.batch = nframes; P.oct_dmax = form ? e->oct_dmax_tab : 0;
    std::vector<uint32_t> count((size_t)nframes * P.cells_per_frame, 0), list((size_t)nframes * P.cell_list_frame_stride, 0);
    for (int f = 0; f < nframes; f++) {
        if (offs[f + 1] < offs[f] || offs[f + 1] - offs[f] > L.key_cap) return ORBHIP_E_CAPACITY;
        for (int i = offs[f]; i < offs[f + 1]; i++) {
            if (xs[i] < 0 || xs[i] >= L.w - 2 * ORB_MINB || ys[i] < 0 || ys[i] >= L.h - 2 * ORB_MINB || scores[i] < 0 || scores[i] > 255) return ORBHIP_E_BADARG;
            const int c = std::min(ys[i] / L.hcell, L.nrows - 1) * L.ncols + std::min(xs[i] / L.wcell, L.ncols - 1);
            uint32_t &n = count[(size_t)f * P.cells_per_frame + L.cell_base + c];
            if ((int)n >= L.cell_cap) return ORBHIP_E_CAPACITY;
            list[(size_t)f * P.cell_list_frame_stride + ((size_t)L.cell_base + c) * L.cell_cap + n++] = ORB_PACK_KEY(xs[i], ys[i], scores[i]);
        }
    }
    HIP_TRY(hipSetDevice(e->ctx->device));
    hipStream_t s = e->ctx->stream;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(P.cell_count, count.data(), sizeof(uint32_t) * count.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(P.cell_list, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice));
    std::vector<int32_t> cnt((size_t)nframes * P.nlevels);
    orb_launch_octree(P, s, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (out_redo) {
        HIP_TRY(hipMemcpy(cnt.data(), P.lvl_count, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));
        for (int f = 0; f < nframes; f++) out_redo[f] = cnt[(size_t)f * P.nlevels + level] < 0 ? 1 : 0;
    }
    if (form) orb_launch_octree(P, s, 2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(cnt.data(), P.lvl_count, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));
    int32_t st = 0;
    HIP_TRY(hipMemcpy(&st, P.status, sizeof(st), hipMemcpyDeviceToHost));
    if (st) { HIP_TRY(hipMemset(P.status, 0, sizeof(int32_t))); return st; }
    for (int f = 0; f < nframes; f++) {
        const int n = cnt[(size_t)f * P.nlevels + level];
        out_counts[f] = n;
        if (n < 0) return ORBHIP_E_HIP;
        const int m = std::min(n, cap);
        if (m > 0) HIP_TRY(hipMemcpy(out_keys + (size_t)f * cap, P.lvl_kp + (size_t)f * P.kps_per_frame + L.kp_base, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    }
    e->last_batch = 0;                                    // the staging arrays no longer belong to an extract call
    return ORBHIP_OK;
}

extern "C" int orbhip_extractor_get_level_keypoints(orbhip_extractor *e, int frame, int level, orbhip_keypoint *out,
                                                    int cap, int32_t *n_out)
{
    if (!e || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch || !n_out) return ORBHIP_E_BADARG;
    const OrbParams &P = e->P;
    const OrbLevel &L = P.lv[level];
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, P.lvl_count + frame * P.nlevels + level, sizeof(n), hipMemcpyDeviceToHost));
    *n_out = n;
    int m = std::min(n, cap);
    if (m > 0 && out) {
        std::vector<uint32_t> k(m); std::vector<float> a(m);
        const size_t off = (size_t)frame * P.kps_per_frame + L.kp_base;
        HIP_TRY(hipMemcpy(k.data(), P.lvl_kp + off, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(a.data(), P.lvl_angle + off, sizeof(float) * m, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) {
            out[i].x = (float)(ORB_KEY_X(k[i]) + ORB_MINB); out[i].y = (float)(ORB_KEY_Y(k[i]) + ORB_MINB);
            out[i].size = L.size; out[i].angle = a[i]; out[i].response = (float)ORB_KEY_S(k[i]);
            out[i].octave = level; out[i].class_id = -1;
        }
    }
    return ORBHIP_OK;
}
