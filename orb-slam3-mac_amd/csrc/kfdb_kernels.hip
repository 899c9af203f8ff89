// kfdb_kernels.hip -- KeyFrameDatabase (reference src/KeyFrameDatabase.cc:35-98, :612-895; L1Scoring::score of
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), batched over queries: what picks the keyframes that enter loop closing, map merging
// (src/LoopClosing.cc:463) and relocalisation (src/Tracking.cc:2634).  The database is a forward table -- per slot a row of ascending word
// ids and double values -- and every query scans all of it; the reference's list order (query words ascending, inverted-list order within
// a word) is recovered as the order by (smallest shared word id, add sequence number).  Six launches per call, all queries in each; no
// workgroup waits on another, the order between them is the stream's:
//   k_kfdb_connected  the connected-keyframe lists scattered into per (query, slot) flags
//   k_kfdb_count      one wave per (query, slot): lanes stride the slot's row and binary-search the query's words (LDS); the shared count by
//                     ballot + popcount and the smallest shared word.  Integers only: order-free
//   k_kfdb_state      one thread per slot walks the queries IN ORDER and applies the reference's rules on (stored query id, words): listed,
//                     marked, touched, the words as this query leaves them, the per-query maximum over the list by atomicMax
//   k_kfdb_score      one wave per listed (query, slot) above the threshold: lanes find the shared terms of 64 row entries at a time, the
//                     double sum takes them one by one in ascending word order (the order is part of the result; no tree sum)
//   k_kfdb_visible    one thread per slot walks the queries in order again: the score a neighbour SHOWS to query q is that of the latest
//                     query <= q of this call and mode that scored it, else the stored one; the stored scores become what the last leaves
//   k_kfdb_finish     one workgroup of 1024 lanes per query: the list sorted by its key in LDS, the scored list compacted in order, the covisibility
//                     accumulation, the stable rank by acc_score (place recognition) and the selections
#include "orb_internal.h"
#include "ctx_internal.h"
#include <climits>
#include <cstring>
#include <vector>

struct orbhip_kfdb {
    orbhip_ctx *ctx;
    int capacity, max_words;
    uint8_t *blob;                                   // one allocation; the pointers below point into it
    int32_t *d_word; double *d_value; int32_t *d_nwords; uint8_t *d_alive; uint32_t *d_seq; int32_t *d_map;
    unsigned long long *d_sq; int32_t *d_sw; float *d_ss;       // [capacity][2]: place recognition, relocalisation
    size_t state_off, state_bytes, meta_off, meta_bytes;
    std::vector<uint8_t> alive;                      // host mirrors: add / erase / clear_map are argument checks, not device round trips
    std::vector<int32_t> map;
    uint32_t next_seq;
};

namespace {

#define KFDB_THREADS 256
#define KFDB_WAVES 4
#define KFDB_FIN_THREADS 1024   // k_kfdb_finish: the LDS sort of up to 4096 keys is what the query waits for
#define KFDB_FIN_WAVES 16
#define KF_LISTED 1u      // in lKFsSharingWords of this query
#define KF_MARKED 2u      // stored query id == the query's id once this query has passed
#define KF_CONN 4u        // in the query's connected list
#define KF_TOUCHED 8u     // words changed without being listed
#define KF_SCORED 16u

struct KfdbArgs {
    const int32_t *word; const double *value; const int32_t *nwords; const uint8_t *alive; const uint32_t *seq; const int32_t *map;
    unsigned long long *sq; int32_t *sw; float *ss; int cap, max_words;
    const orbhip_kfdb_query *query; int queries; const int32_t *qword; const double *qvalue; const int32_t *qn; int q_stride;
    const int32_t *conn; const int32_t *nconn; int max_conn;
    int32_t *w_cnt, *w_first, *w_words, *w_maxc, *w_firstidx; uint8_t *w_flags; float *w_score;
    const int32_t *neigh; int n_cand; const int32_t *bad; int n_bad; int max_list, list_p2;
    int32_t *counts; orbhip_kfdb_entry *list; orbhip_kfdb_candidate *scored; int32_t *loop, *merge, *ncand, *reloc, *nreloc, *status;
};

// the words of query q, or -1 when its count cannot be used
__device__ __forceinline__ int kfdb_qlen(const KfdbArgs &a, int q)
{
    const int n = a.qn[q];
    return (n < 0 || n > a.max_words || n > a.q_stride) ? -1 : n;
}
__device__ __forceinline__ int kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }

// index of w in the ascending list p[0, n), or -1
template <typename P> __device__ __forceinline__ int kfdb_find(P p, int n, int w)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (p[mid] < w) lo = mid + 1; else hi = mid; }
    return (lo < n && p[lo] == w) ? lo : -1;
}

__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_connected(KfdbArgs a)
{
    const int q = blockIdx.y, i = blockIdx.x * KFDB_THREADS + threadIdx.x;
    if (a.query[q].mode != ORBHIP_KFDB_PLACE) return;
    int n = a.nconn[q];
    if (n > a.max_conn) n = a.max_conn;
    if (i >= n) return;
    const int s = a.conn[(size_t)q * a.max_conn + i];
    if (s >= 0 && s < a.cap) a.w_flags[(size_t)q * a.cap + s] = KF_CONN;
}

__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_count(KfdbArgs a)
{
    __shared__ int32_t s_q[ORBHIP_KFDB_MAX_WORDS];
    const int q = blockIdx.y, lane = threadIdx.x & 63, slot = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6);
    const int nq = kfdb_qlen(a, q);                                             // <= max_words <= 4096
    for (int i = threadIdx.x; i < nq; i += KFDB_THREADS) s_q[i] = a.qword[(size_t)q * a.q_stride + i];
    __syncthreads();
    if (slot >= a.cap) return;
    int c = 0, first = INT_MAX;
    if (nq > 0 && a.alive[slot]) {
        const int n = min(a.nwords[slot], a.max_words);
        const int32_t *row = a.word + (size_t)slot * a.max_words;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool hit = false;
            if (i < n) { const int w = row[i]; hit = kfdb_find(s_q, nq, w) >= 0; if (hit) first = min(first, w); }
            c += __popcll(__ballot(hit));
        }
        for (int m = 32; m; m >>= 1) first = min(first, __shfl_xor(first, m, 64));
    }
    if (lane == 0) { a.w_cnt[(size_t)q * a.cap + slot] = c; a.w_first[(size_t)q * a.cap + slot] = first; }
}

__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_state(KfdbArgs a)
{
    const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
    const bool live = s < a.cap;                                                // no early exit: the wave reduces the maximum together
    unsigned long long sq[2] = {0, 0};
    int sw[2] = {0, 0};
    if (live) { sq[0] = a.sq[2 * s]; sq[1] = a.sq[2 * s + 1]; sw[0] = a.sw[2 * s]; sw[1] = a.sw[2 * s + 1]; }
    for (int q = 0; q < a.queries; q++) {
        const size_t at = live ? (size_t)q * a.cap + s : 0;
        const int c = live ? a.w_cnt[at] : 0;
        const unsigned long long id = a.query[q].id;
        const bool reloc = a.query[q].mode == ORBHIP_KFDB_RELOC;
        unsigned f = live ? a.w_flags[at] & KF_CONN : 0u;
        unsigned long long stored = reloc ? sq[1] : sq[0];
        int words = reloc ? sw[1] : sw[0];
        if (c > 0) {
            if (stored != id) {
                if (!reloc && f) { words = 1; f |= KF_TOUCHED; }               // reset at every encounter, never marked (:635-645)
                else { stored = id; words = c; f |= KF_LISTED; }
            } else { words += c; f |= KF_TOUCHED; }
        }
        if (reloc) { sq[1] = stored; sw[1] = words; } else { sq[0] = stored; sw[0] = words; }
        if (stored == id) f |= KF_MARKED;
        if (live) { a.w_flags[at] = (uint8_t)f; a.w_words[at] = words; }
        int mx = (f & KF_LISTED) ? words : 0;                                   // a listed slot has words >= 1
        for (int m = 32; m; m >>= 1) mx = max(mx, __shfl_xor(mx, m, 64));
        if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(a.w_maxc + q, mx);     // one atomic per wave, not one per slot
    }
    if (live) { a.sq[2 * s] = sq[0]; a.sq[2 * s + 1] = sq[1]; a.sw[2 * s] = sw[0]; a.sw[2 * s + 1] = sw[1]; }
}

__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_score(KfdbArgs a)
{
    const int q = blockIdx.y, lane = threadIdx.x & 63, slot = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6);
    if (slot >= a.cap) return;
    const size_t at = (size_t)q * a.cap + slot;
    if (!(a.w_flags[at] & KF_LISTED) || a.w_words[at] <= kfdb_min_common(a.w_maxc[q])) return;       // wave-uniform
    const int nq = kfdb_qlen(a, q), n = min(a.nwords[slot], a.max_words);       // a listed slot has nq > 0
    const int32_t *qw = a.qword + (size_t)q * a.q_stride, *row = a.word + (size_t)slot * a.max_words;
    const double *qv = a.qvalue + (size_t)q * a.q_stride, *val = a.value + (size_t)slot * a.max_words;
    double sum = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        double term = 0.0;
        bool hit = false;
        if (i < n) {
            const int j = kfdb_find(qw, nq, row[i]);
            if (j >= 0) { const double vi = qv[j], wi = val[i]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); hit = true; }
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {                                                          // ascending word order: one addition per shared word
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            // the lane index is wave-uniform: two v_readlane, no trip through LDS
            sum += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(term), l), __builtin_amdgcn_readlane(__double2loint(term), l));
        }
    }
    if (lane == 0) a.w_score[at] = (float)(-sum / 2.0);
}

__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_visible(KfdbArgs a)
{
    const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
    if (s >= a.cap) return;
    float ss[2] = {a.ss[2 * s], a.ss[2 * s + 1]};
    for (int q = 0; q < a.queries; q++) {
        const size_t at = (size_t)q * a.cap + s;
        const int m = a.query[q].mode == ORBHIP_KFDB_RELOC ? 1 : 0;
        const unsigned f = a.w_flags[at];
        if ((f & KF_LISTED) && a.w_words[at] > kfdb_min_common(a.w_maxc[q])) {
            const float v = a.w_score[at];
            if (m) ss[1] = v; else ss[0] = v;
            a.w_flags[at] = (uint8_t)(f | KF_SCORED);
        }
        a.w_score[at] = m ? ss[1] : ss[0];
    }
    a.ss[2 * s] = ss[0]; a.ss[2 * s + 1] = ss[1];
}

// ascending bitonic sort of key[0, p2) (p2 a power of two) with its payload
__device__ void kfdb_sort(unsigned long long *key, int32_t *pay, int p2)
{
    for (int k = 2; k <= p2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < p2; i += KFDB_FIN_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long ka = key[i], kb = key[x];
                    if ((ka > kb) == ((i & k) == 0)) { key[i] = kb; key[x] = ka; const int32_t t = pay[i]; pay[i] = pay[x]; pay[x] = t; }
                }
            }
            __syncthreads();
        }
}

// position of this thread's element among the flagged ones of the block, in thread order, counted on from `running`; every thread calls
__device__ __forceinline__ int kfdb_compact(bool flag, int &running, int *s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int off = running, total = 0;
    for (int w = 0; w < KFDB_FIN_WAVES; w++) { if (w < wave) off += s_w[w]; total += s_w[w]; }
    const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();
    running += total;
    return pos;
}

// a float as an unsigned that orders the same way (+0 and -0 are one value to operator>)
__device__ __forceinline__ uint32_t kfdb_ordered(float v)
{
    uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(KFDB_FIN_THREADS) k_kfdb_finish(KfdbArgs a)
{
    extern __shared__ unsigned long long s_dyn[];
    unsigned long long *s_key = s_dyn;                                         // [list_p2]
    int32_t *s_idx = reinterpret_cast<int32_t *>(s_dyn + a.list_p2);           // [list_p2]
    int32_t *s_sc = s_idx + a.list_p2;                                         // [list_p2] scored slots in list order
    __shared__ int s_n, s_nl, s_w[KFDB_FIN_WAVES];
    __shared__ float s_red[KFDB_FIN_THREADS];
    const int q = blockIdx.x, tid = threadIdx.x;
    const orbhip_kfdb_query Q = a.query[q];
    const bool reloc = Q.mode == ORBHIP_KFDB_RELOC, detect = a.neigh != nullptr;
    const size_t qrow = (size_t)q * a.cap;
    int32_t *counts = a.counts + 4 * (size_t)q;
    if (tid == 0) {                                                             // thread 0 alone writes the counts, first and last
        s_n = 0; s_nl = 0;
        counts[0] = 0; counts[1] = 0; counts[2] = 0; counts[3] = 0;
        if (detect) { a.ncand[2 * q] = 0; a.ncand[2 * q + 1] = 0; a.nreloc[q] = 0; }
    }
    __syncthreads();
    if (kfdb_qlen(a, q) < 0) { if (tid == 0) atomicExch(a.status, ORBHIP_E_CAPACITY); return; }
    // the sharing list, and behind it the slots this query touched without listing them
    for (int s = tid; s < a.cap; s += KFDB_FIN_THREADS) {
        const unsigned f = a.w_flags[qrow + s];
        if (f & (KF_LISTED | KF_TOUCHED)) {
            const int pos = atomicAdd(&s_n, 1);
            if (f & KF_LISTED) atomicAdd(&s_nl, 1);
            if (pos < a.max_list) {                                             // max_list <= list_p2
                s_key[pos] = ((f & KF_LISTED) ? 0ull : 1ull << 63) | ((unsigned long long)(uint32_t)a.w_first[qrow + s] << 32) | a.seq[s];
                s_idx[pos] = s;
            }
        }
    }
    __syncthreads();
    const int n = s_n, nl = s_nl;
    if (n > a.max_list) { if (tid == 0) atomicExch(a.status, ORBHIP_E_CAPACITY); return; }
    if (n == 0) return;
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    for (int i = n + tid; i < p2; i += KFDB_FIN_THREADS) { s_key[i] = ~0ull; s_idx[i] = -1; }
    __syncthreads();
    kfdb_sort(s_key, s_idx, p2);
    const int maxc = a.w_maxc[q];
    int ns = 0;
    for (int base = 0; base < n; base += KFDB_FIN_THREADS) {
        const int i = base + tid;
        bool sc = false;
        int s = -1;
        if (i < n) {
            s = s_idx[i];
            sc = i < nl && (a.w_flags[qrow + s] & KF_SCORED);
            orbhip_kfdb_entry e;
            e.slot = s; e.words = a.w_words[qrow + s]; e.scored = sc ? 1 : 0; e.score = sc ? a.w_score[qrow + s] : 0.f;
            a.list[(size_t)q * a.max_list + i] = e;
        }
        const int pos = kfdb_compact(sc, ns, s_w);
        if (sc) s_sc[pos] = s;
    }
    if (tid == 0) { counts[0] = nl; counts[1] = maxc; counts[2] = ns; counts[3] = n - nl; }
    if (!detect || ns == 0) return;
    __syncthreads();
    // accumulation over the first 10 covisibility neighbours (:693-718, :846-871); s_key / s_idx are free again
    float best_acc = 0.f;
    for (int j = tid; j < ns; j += KFDB_FIN_THREADS) {
        const int s = s_sc[j];
        const float si = a.w_score[qrow + s];
        float best = si, acc = si;
        int bs = s;
        for (int k = 0; k < ORBHIP_KFDB_NEIGHBOURS; k++) {
            const int nb = a.neigh[(size_t)s * ORBHIP_KFDB_NEIGHBOURS + k];
            if (nb < 0 || nb >= a.cap || !(a.w_flags[qrow + nb] & KF_MARKED)) continue;
            const float v = a.w_score[qrow + nb];
            acc += v;
            if (v > best) { bs = nb; best = v; }
        }
        orbhip_kfdb_candidate c;
        c.slot = s; c.score = si; c.acc_score = acc; c.best_slot = bs;
        a.scored[(size_t)q * a.max_list + j] = c;
        s_key[j] = ((unsigned long long)(~kfdb_ordered(acc)) << 32) | (uint32_t)j;      // acc_score descending, then list order
        s_idx[j] = bs;
        if (acc > best_acc) best_acc = acc;
    }
    s_red[tid] = best_acc;
    __syncthreads();
    for (int m = KFDB_FIN_THREADS / 2; m; m >>= 1) { if (tid < m && s_red[tid + m] > s_red[tid]) s_red[tid] = s_red[tid + m]; __syncthreads(); }
    best_acc = s_red[0];
    int32_t *firstidx = a.w_firstidx + qrow;                                    // INT_MAX-like everywhere on entry
    if (reloc) {
        const float keep = 0.75f * best_acc;
        for (int j = tid; j < ns; j += KFDB_FIN_THREADS) {
            const int bs = s_idx[j];
            const bool pass = a.scored[(size_t)q * a.max_list + j].acc_score > keep && a.map[bs] == Q.map_id;
            s_sc[j] = pass ? 1 : 0;
            if (pass) atomicMin(firstidx + bs, j);
        }
        __syncthreads();
        int nr = 0;
        for (int base = 0; base < ns; base += KFDB_FIN_THREADS) {
            const int j = base + tid;
            const bool take = j < ns && s_sc[j] && atomicMin(firstidx + s_idx[j], INT_MAX) == j;
            const int pos = kfdb_compact(take, nr, s_w);
            if (take) a.reloc[(size_t)q * a.max_list + pos] = s_idx[j];
        }
        if (tid == 0) a.nreloc[q] = nr;
        return;
    }
    p2 = 1;
    while (p2 < ns) p2 <<= 1;
    for (int i = ns + tid; i < p2; i += KFDB_FIN_THREADS) { s_key[i] = ~0ull; s_idx[i] = -1; }
    __syncthreads();
    kfdb_sort(s_key, s_idx, p2);
    for (int r = tid; r < ns; r += KFDB_FIN_THREADS) atomicMin(firstidx + s_idx[r], r);
    __syncthreads();
    int nloop = 0, nmerge = 0;
    for (int base = 0; base < ns; base += KFDB_FIN_THREADS) {
        const int r = base + tid;
        bool lp = false, mg = false;
        int bs = -1;
        if (r < ns) {
            bs = s_idx[r];
            if (atomicMin(firstidx + bs, INT_MAX) == r) {                       // first seen in rank order (spAlreadyAddedKF)
                const int m = a.map[bs];
                if (m == Q.map_id) lp = true;
                else { mg = true; for (int b = 0; b < a.n_bad; b++) if (a.bad[b] == m) mg = false; }
            }
        }
        const int pl = kfdb_compact(lp, nloop, s_w);
        if (lp && pl < a.n_cand) a.loop[(size_t)q * a.n_cand + pl] = bs;
        const int pm = kfdb_compact(mg, nmerge, s_w);
        if (mg && pm < a.n_cand) a.merge[(size_t)q * a.n_cand + pm] = bs;
    }
    if (tid == 0) { a.ncand[2 * q] = min(nloop, a.n_cand); a.ncand[2 * q + 1] = min(nmerge, a.n_cand); }
}

// add: the row copied from device arrays (src_word != nullptr; the count read on the device) or already in place (add_host)
__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_add(int32_t *word, double *value, int32_t *nwords, uint8_t *alive, uint32_t *seq, int32_t *map,
        int max_words, int slot, int map_id, uint32_t sequence, const int32_t *src_word, const double *src_value, const int32_t *src_n, int n_host,
        int32_t *status)
{
    const int n = src_n ? *src_n : n_host;
    if (n < 0 || n > max_words) { if (threadIdx.x == 0) { atomicExch(status, ORBHIP_E_CAPACITY); alive[slot] = 0; nwords[slot] = 0; } return; }
    if (src_word)
        for (int i = threadIdx.x; i < n; i += KFDB_THREADS) { word[(size_t)slot * max_words + i] = src_word[i]; value[(size_t)slot * max_words + i] = src_value[i]; }
    if (threadIdx.x == 0) { nwords[slot] = n; alive[slot] = 1; seq[slot] = sequence; map[slot] = map_id; }
}
__global__ void k_kfdb_erase(uint8_t *alive, int slot) { alive[slot] = 0; }
__global__ void __launch_bounds__(KFDB_THREADS) k_kfdb_clear_map(uint8_t *alive, const int32_t *map, int cap, int map_id)
{
    const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
    if (s < cap && alive[s] && map[s] == map_id) alive[s] = 0;
}
__global__ void k_kfdb_reset_slot(unsigned long long *sq, int32_t *sw, float *ss, int slot)
{
    sq[2 * slot] = 0; sq[2 * slot + 1] = 0; sw[2 * slot] = 0; sw[2 * slot + 1] = 0; ss[2 * slot] = 0.f; ss[2 * slot + 1] = 0.f;
}

int kfdb_fail(int code, const char *msg) { orbhip_set_last_error_internal(msg); return code; }
int kfdb_enter(orbhip_kfdb *db, const char *null_msg)
{
    if (!db) return kfdb_fail(ORBHIP_E_BADARG, null_msg);
    if (hipSetDevice(orbhip_ctx_device_internal(db->ctx)) != hipSuccess) return kfdb_fail(ORBHIP_E_HIP, "hipSetDevice");
    return ORBHIP_OK;
}
int kfdb_launched(const char *msg) { return hipGetLastError() != hipSuccess ? kfdb_fail(ORBHIP_E_HIP, msg) : ORBHIP_OK; }

}  // namespace

orbhip_ctx *orbhip_kfdb_ctx_internal(orbhip_kfdb *db) { return db->ctx; }
int orbhip_kfdb_max_words_internal(orbhip_kfdb *db) { return db->max_words; }

extern "C" int orbhip_kfdb_create(orbhip_ctx *ctx, int capacity, int max_words, orbhip_kfdb **out)
{
    if (!ctx || !out) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_create: ctx or out is NULL");
    if (capacity < 1) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_create: capacity < 1");
    if (max_words < 1 || max_words > ORBHIP_KFDB_MAX_WORDS) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_create: max_words outside 1..4096");
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return kfdb_fail(ORBHIP_E_HIP, "hipSetDevice");
    const size_t C = (size_t)capacity, W = (size_t)max_words;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_val = take(8 * C * W), o_word = take(4 * C * W);
    const size_t o_meta = off, o_nw = take(4 * C), o_alive = take(C), o_seq = take(4 * C), o_map = take(4 * C);
    const size_t o_state = off, o_sq = take(16 * C), o_sw = take(8 * C), o_ss = take(8 * C);
    orbhip_kfdb *db = new orbhip_kfdb();
    db->ctx = ctx; db->capacity = capacity; db->max_words = max_words; db->next_seq = 0;
    if (hipMalloc((void **)&db->blob, off) != hipSuccess) { delete db; return kfdb_fail(ORBHIP_E_HIP, "orbhip_kfdb_create: hipMalloc"); }
    db->d_value = (double *)(db->blob + o_val); db->d_word = (int32_t *)(db->blob + o_word); db->d_nwords = (int32_t *)(db->blob + o_nw);
    db->d_alive = db->blob + o_alive; db->d_seq = (uint32_t *)(db->blob + o_seq); db->d_map = (int32_t *)(db->blob + o_map);
    db->d_sq = (unsigned long long *)(db->blob + o_sq); db->d_sw = (int32_t *)(db->blob + o_sw); db->d_ss = (float *)(db->blob + o_ss);
    db->meta_off = o_meta; db->meta_bytes = o_state - o_meta; db->state_off = o_state; db->state_bytes = off - o_state;
    db->alive.assign(C, 0); db->map.assign(C, 0);
    if (hipMemsetAsync(db->blob, 0, off, orbhip_ctx_stream_internal(ctx)) != hipSuccess) {
        (void)hipFree(db->blob); delete db; return kfdb_fail(ORBHIP_E_HIP, "orbhip_kfdb_create: hipMemsetAsync");
    }
    *out = db;
    return ORBHIP_OK;
}

extern "C" void orbhip_kfdb_destroy(orbhip_kfdb *db)
{
    if (!db) return;
    if (hipSetDevice(orbhip_ctx_device_internal(db->ctx)) == hipSuccess) (void)hipStreamSynchronize(orbhip_ctx_stream_internal(db->ctx));
    (void)hipFree(db->blob);
    delete db;
}

static int kfdb_add(orbhip_kfdb *db, const char *who_null, int slot, int map_id, const int32_t *d_word, const double *d_value, const int32_t *d_n,
                    const int32_t *h_word, const double *h_value, int n_host)
{
    if (int rc = kfdb_enter(db, who_null)) return rc;
    if (slot < 0 || slot >= db->capacity) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb_add: slot outside the capacity");
    if (db->alive[slot]) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_add: slot is alive");
    hipStream_t st = orbhip_ctx_stream_internal(db->ctx);
    if (!d_n) {
        if (n_host < 0) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_add_host: nwords < 0");
        if (n_host > db->max_words) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb_add_host: nwords > max_words");
        if (n_host && (!h_word || !h_value)) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_add_host: word or value is NULL");
        if (n_host) {
            // straight from the caller's pageable arrays, which it may free on return: the runtime stages a pageable host-to-device copy
            // before hipMemcpyAsync returns -- the assumption host_entry.hip's pageable mode rests on as well.  The context's page-locked
            // arena is no alternative here: a call that does not synchronise cannot know when an earlier copy out of it has finished
            ORB_HIP_TRY(hipMemcpyAsync(db->d_word + (size_t)slot * db->max_words, h_word, 4 * (size_t)n_host, hipMemcpyHostToDevice, st));
            ORB_HIP_TRY(hipMemcpyAsync(db->d_value + (size_t)slot * db->max_words, h_value, 8 * (size_t)n_host, hipMemcpyHostToDevice, st));
        }
    } else if (!d_word || !d_value) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_add_device: d_word or d_value is NULL");
    hipLaunchKernelGGL(k_kfdb_add, dim3(1), dim3(KFDB_THREADS), 0, st, db->d_word, db->d_value, db->d_nwords, db->d_alive, db->d_seq, db->d_map,
                       db->max_words, slot, map_id, db->next_seq, d_n ? d_word : nullptr, d_value, d_n, n_host, orbhip_ctx_status_internal(db->ctx));
    if (int rc = kfdb_launched("orbhip_kfdb_add: launch")) return rc;
    db->next_seq++;
    db->alive[slot] = 1; db->map[slot] = map_id;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_add_device(orbhip_kfdb *db, int slot, int map_id, const int32_t *d_word, const double *d_value, const int32_t *d_nwords)
{
    if (db && !d_nwords) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_add_device: d_nwords is NULL");
    return kfdb_add(db, "orbhip_kfdb_add_device: db is NULL", slot, map_id, d_word, d_value, d_nwords, nullptr, nullptr, 0);
}

extern "C" int orbhip_kfdb_add_host(orbhip_kfdb *db, int slot, int map_id, const int32_t *word, const double *value, int nwords)
{
    return kfdb_add(db, "orbhip_kfdb_add_host: db is NULL", slot, map_id, nullptr, nullptr, nullptr, word, value, nwords);
}

extern "C" int orbhip_kfdb_erase(orbhip_kfdb *db, int slot)
{
    if (int rc = kfdb_enter(db, "orbhip_kfdb_erase: db is NULL")) return rc;
    if (slot < 0 || slot >= db->capacity) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb_erase: slot outside the capacity");
    if (!db->alive[slot]) return ORBHIP_OK;
    hipLaunchKernelGGL(k_kfdb_erase, dim3(1), dim3(1), 0, orbhip_ctx_stream_internal(db->ctx), db->d_alive, slot);
    if (int rc = kfdb_launched("orbhip_kfdb_erase: launch")) return rc;
    db->alive[slot] = 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_clear_map(orbhip_kfdb *db, int map_id)
{
    if (int rc = kfdb_enter(db, "orbhip_kfdb_clear_map: db is NULL")) return rc;
    hipLaunchKernelGGL(k_kfdb_clear_map, dim3((db->capacity + KFDB_THREADS - 1) / KFDB_THREADS), dim3(KFDB_THREADS), 0,
                       orbhip_ctx_stream_internal(db->ctx), db->d_alive, db->d_map, db->capacity, map_id);
    if (int rc = kfdb_launched("orbhip_kfdb_clear_map: launch")) return rc;
    for (int s = 0; s < db->capacity; s++) if (db->alive[s] && db->map[s] == map_id) db->alive[s] = 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_clear(orbhip_kfdb *db)
{
    if (int rc = kfdb_enter(db, "orbhip_kfdb_clear: db is NULL")) return rc;
    ORB_HIP_TRY(hipMemsetAsync(db->blob + db->meta_off, 0, db->meta_bytes + db->state_bytes, orbhip_ctx_stream_internal(db->ctx)));
    std::fill(db->alive.begin(), db->alive.end(), 0);
    db->next_seq = 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_reset_slot(orbhip_kfdb *db, int slot)
{
    if (int rc = kfdb_enter(db, "orbhip_kfdb_reset_slot: db is NULL")) return rc;
    if (slot < 0 || slot >= db->capacity) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb_reset_slot: slot outside the capacity");
    hipLaunchKernelGGL(k_kfdb_reset_slot, dim3(1), dim3(1), 0, orbhip_ctx_stream_internal(db->ctx), db->d_sq, db->d_sw, db->d_ss, slot);
    return kfdb_launched("orbhip_kfdb_reset_slot: launch");
}

extern "C" int orbhip_kfdb_get_state_host(orbhip_kfdb *db, int first, int n, orbhip_kfdb_slot_state *out)
{
    if (int rc = kfdb_enter(db, "orbhip_kfdb_get_state_host: db is NULL")) return rc;
    if (n < 0 || (n && !out)) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_get_state_host: n < 0 or out is NULL");
    if (first < 0 || first > db->capacity || n > db->capacity - first) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb_get_state_host: slots outside the capacity");
    if (n == 0) return ORBHIP_OK;
    ORB_HIP_TRY(hipStreamSynchronize(orbhip_ctx_stream_internal(db->ctx)));
    const size_t N = (size_t)n;
    std::vector<unsigned long long> sq(2 * N); std::vector<int32_t> sw(2 * N), nw(N), mp(N); std::vector<float> ss(2 * N);
    std::vector<uint8_t> al(N); std::vector<uint32_t> sn(N);
    ORB_HIP_TRY(hipMemcpy(sq.data(), db->d_sq + 2 * (size_t)first, 16 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(sw.data(), db->d_sw + 2 * (size_t)first, 8 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(ss.data(), db->d_ss + 2 * (size_t)first, 8 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(nw.data(), db->d_nwords + first, 4 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(mp.data(), db->d_map + first, 4 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(sn.data(), db->d_seq + first, 4 * N, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(al.data(), db->d_alive + first, N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
        orbhip_kfdb_slot_state &o = out[i];
        for (int m = 0; m < 2; m++) { o.query[m] = sq[2 * i + m]; o.words[m] = sw[2 * i + m]; o.score[m] = ss[2 * i + m]; }
        o.n_words = nw[i]; o.alive = al[i]; o.map_id = mp[i]; o.sequence = sn[i];
    }
    return ORBHIP_OK;
}

int orbhip_kfdb_launch_internal(orbhip_kfdb *db, const char *who, const orbhip_kfdb_query *query, const orbhip_kfdb_query *d_query, int queries,
        const int32_t *d_qword, const double *d_qvalue, const int32_t *d_qn, int q_stride, const int32_t *d_connected,
        const int32_t *d_nconnected, int max_connected, const int32_t *d_neighbours, int n_candidates, const int32_t *bad_maps, int n_bad,
        int max_list, int32_t *d_counts, orbhip_kfdb_entry *d_list, orbhip_kfdb_candidate *d_scored, int32_t *d_loop, int32_t *d_merge,
        int32_t *d_ncand, int32_t *d_reloc, int32_t *d_nreloc)
{
    (void)who;
    if (int rc = kfdb_enter(db, "orbhip_kfdb: db is NULL")) return rc;
    if (!query || queries < 1) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb: query is NULL or queries < 1");
    if (!d_qword || !d_qvalue || !d_qn || q_stride < 1) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb: d_qword, d_qvalue or d_qn is NULL, or q_stride < 1");
    if (max_connected < 0 || (max_connected && (!d_connected || !d_nconnected))) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb: max_connected < 0, or d_connected / d_nconnected is NULL");
    if (!d_counts || !d_list) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb: d_counts or d_list is NULL");
    if (max_list < 1 || max_list > ORBHIP_KFDB_MAX_LIST) return kfdb_fail(ORBHIP_E_CAPACITY, "orbhip_kfdb: max_list outside 1..4096");
    for (int q = 0; q < queries; q++)
        if (query[q].mode != ORBHIP_KFDB_PLACE && query[q].mode != ORBHIP_KFDB_RELOC) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb: query mode is neither ORBHIP_KFDB_PLACE nor ORBHIP_KFDB_RELOC");
    const bool detect = d_neighbours != nullptr;
    if (detect) {
        if (n_candidates < 0) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_detect_device: n_candidates < 0");
        if (n_bad < 0 || (n_bad && !bad_maps)) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_detect_device: n_bad < 0 or bad_maps is NULL");
        if (!d_scored || !d_ncand || !d_reloc || !d_nreloc || (n_candidates && (!d_loop || !d_merge))) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_detect_device: an output (d_scored, d_loop, d_merge, d_ncand, d_reloc, d_nreloc) is NULL");
    }
    const size_t QC = (size_t)queries * db->capacity;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_flags = take(QC), o_maxc = take(4 * (size_t)queries);        // zeroed together
    const size_t zero_end = off;
    const size_t o_fi = take(4 * QC), o_cnt = take(4 * QC), o_first = take(4 * QC), o_words = take(4 * QC), o_score = take(4 * QC);
    const size_t o_query = take(sizeof(orbhip_kfdb_query) * (size_t)queries), o_bad = take(4 * (size_t)(n_bad > 0 ? n_bad : 1));
    uint8_t *w = (uint8_t *)orbhip_ctx_work_internal(db->ctx, off + 256);
    if (!w) return ORBHIP_E_HIP;
    hipStream_t st = orbhip_ctx_stream_internal(db->ctx);
    ORB_HIP_TRY(hipMemsetAsync(w, 0, zero_end, st));
    if (detect) ORB_HIP_TRY(hipMemsetAsync(w + o_fi, 0x7f, 4 * QC, st));
    // `query` and `bad_maps` are the caller's pageable memory, reusable on return: staged by the runtime before the call returns (see kfdb_add)
    if (!d_query) ORB_HIP_TRY(hipMemcpyAsync(w + o_query, query, sizeof(orbhip_kfdb_query) * (size_t)queries, hipMemcpyHostToDevice, st));
    if (detect && n_bad) ORB_HIP_TRY(hipMemcpyAsync(w + o_bad, bad_maps, 4 * (size_t)n_bad, hipMemcpyHostToDevice, st));
    KfdbArgs a;
    memset(&a, 0, sizeof(a));
    a.word = db->d_word; a.value = db->d_value; a.nwords = db->d_nwords; a.alive = db->d_alive; a.seq = db->d_seq; a.map = db->d_map;
    a.sq = db->d_sq; a.sw = db->d_sw; a.ss = db->d_ss; a.cap = db->capacity; a.max_words = db->max_words;
    a.query = d_query ? d_query : (const orbhip_kfdb_query *)(w + o_query); a.queries = queries;
    a.qword = d_qword; a.qvalue = d_qvalue; a.qn = d_qn; a.q_stride = q_stride;
    a.conn = d_connected; a.nconn = d_nconnected; a.max_conn = max_connected;
    a.w_flags = w + o_flags; a.w_maxc = (int32_t *)(w + o_maxc); a.w_firstidx = (int32_t *)(w + o_fi); a.w_cnt = (int32_t *)(w + o_cnt);
    a.w_first = (int32_t *)(w + o_first); a.w_words = (int32_t *)(w + o_words); a.w_score = (float *)(w + o_score);
    a.neigh = d_neighbours; a.n_cand = n_candidates; a.bad = (const int32_t *)(w + o_bad); a.n_bad = detect ? n_bad : 0;
    a.max_list = max_list;
    a.list_p2 = 1;
    while (a.list_p2 < max_list) a.list_p2 <<= 1;
    a.counts = d_counts; a.list = d_list; a.scored = d_scored; a.loop = d_loop; a.merge = d_merge; a.ncand = d_ncand; a.reloc = d_reloc; a.nreloc = d_nreloc;
    a.status = orbhip_ctx_status_internal(db->ctx);
    const size_t lds = 16 * (size_t)a.list_p2;                                  // keys 8 + payload 4 + scored list 4 bytes per entry: <= 64 KB
    if (orb_lds_optin(reinterpret_cast<const void *>(k_kfdb_finish), orbhip_ctx_device_internal(db->ctx), lds)) return ORBHIP_E_HIP;
    const unsigned slot_blocks = (unsigned)((db->capacity + KFDB_WAVES - 1) / KFDB_WAVES), cap_blocks = (unsigned)((db->capacity + KFDB_THREADS - 1) / KFDB_THREADS);
    if (max_connected) hipLaunchKernelGGL(k_kfdb_connected, dim3((max_connected + KFDB_THREADS - 1) / KFDB_THREADS, queries), dim3(KFDB_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_kfdb_count, dim3(slot_blocks, queries), dim3(KFDB_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_kfdb_state, dim3(cap_blocks), dim3(KFDB_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_kfdb_score, dim3(slot_blocks, queries), dim3(KFDB_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_kfdb_visible, dim3(cap_blocks), dim3(KFDB_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_kfdb_finish, dim3(queries), dim3(KFDB_FIN_THREADS), lds, st, a);
    return kfdb_launched("orbhip_kfdb: launch");
}

extern "C" int orbhip_kfdb_score_device(orbhip_kfdb *db, const orbhip_kfdb_query *query, int queries, const int32_t *d_qword, const double *d_qvalue,
        const int32_t *d_qn, int q_stride, const int32_t *d_connected, const int32_t *d_nconnected, int max_connected, int max_list,
        int32_t *d_counts, orbhip_kfdb_entry *d_list)
{
    return orbhip_kfdb_launch_internal(db, "orbhip_kfdb_score_device", query, nullptr, queries, d_qword, d_qvalue, d_qn, q_stride, d_connected, d_nconnected,
                                       max_connected, nullptr, 0, nullptr, 0, max_list, d_counts, d_list, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int orbhip_kfdb_detect_device(orbhip_kfdb *db, const orbhip_kfdb_query *query, int queries, const int32_t *d_qword, const double *d_qvalue,
        const int32_t *d_qn, int q_stride, const int32_t *d_connected, const int32_t *d_nconnected, int max_connected,
        const int32_t *d_neighbours, int n_candidates, const int32_t *bad_maps, int n_bad, int max_list,
        int32_t *d_counts, orbhip_kfdb_entry *d_list, orbhip_kfdb_candidate *d_scored, int32_t *d_loop, int32_t *d_merge, int32_t *d_ncand,
        int32_t *d_reloc, int32_t *d_nreloc)
{
    if (db && !d_neighbours) return kfdb_fail(ORBHIP_E_BADARG, "orbhip_kfdb_detect_device: d_neighbours is NULL");
    return orbhip_kfdb_launch_internal(db, "orbhip_kfdb_detect_device", query, nullptr, queries, d_qword, d_qvalue, d_qn, q_stride, d_connected, d_nconnected,
                                       max_connected, d_neighbours, n_candidates, bad_maps, n_bad, max_list, d_counts, d_list, d_scored, d_loop, d_merge,
                                       d_ncand, d_reloc, d_nreloc);
}
