// orb_kernels.hip -- two stages of the ORB front-end (ORBextractor::operator(), reference src/ORBextractor.cc:1068-1150):
// DistributeOctTree (k_octree, k_octree_tab, k_octree_redo) and the output assembly (k_assemble).  The other stages have a
// file each: pyramid_kernels.hip, fast_kernels.hip, blur_kernels.hip, desc_kernels.hip.
//
// One launch processes a whole batch of frames; blockIdx carries (list|frame).  Integer work throughout, no MFMA.
// Wave = 64 lanes everywhere.  Compile: hipcc --offload-arch=gfx950 -ffp-contract=off.
#include "orb_internal.h"
#include "wave_dpp.h"

#define WAVE 64

// ----------------------------------------------------------------------------------
// helpers
// ----------------------------------------------------------------------------------
// Exclusive scan of one int per thread over a 256-thread block. `wsum` = 8 ints of LDS.
// Returns exclusive prefix; *total = block sum.  Contains two __syncthreads().
__device__ __forceinline__ int block_excl_scan256(int v, int *wsum, int *total)
{
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
    int inc = wave_incl_scan(v);
    if (lane == WAVE - 1) wsum[wid] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        int s = wsum[w];
        if (w < wid) base += s;
    }
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + inc - v;
}

// ----------------------------------------------------------------------------------
// A5  DistributeOctTree (ORBextractor.cc:537-761), one 256-thread workgroup per
// (frame, level), node state resident in LDS.
//
// Reformulation (bit-identical to the oracle's list-based restatement):
//  * every node's vKeys is a subsequence of the level's candidate list in original
//    order (DivideNode pushes in order), so a per-key node id replaces the key vectors;
//  * the std::list order is an explicit position: a step that splits the set `proc`
//    in processing order o=0..m-1 yields  [children(o=m-1) n4..n1, ..., children(o=0)
//    n4..n1, surviving old nodes in old order]  (push_front semantics);
//  * full pass: proc = all nodes with >1 key, processing order = list order;
//  * final phase (ORBextractor.cc:665-735): candidates = children with >1 key created by
//    the previous step, processing order = (size desc, creation desc) == (size desc,
//    list position asc); stop after the first split that reaches N nodes.  The
//    reference breaks ties by node address (non-deterministic); oracle and
//    kernel use creation order -- documented deviation.
// ----------------------------------------------------------------------------------
struct OctLds {
    uint32_t *cc;        // [NC*4] child key counts
    int *ord;            // [NC] processing order of node p, or -1
    int *by_ord;         // [NC] node at order o
    int *excl;           // [NC] exclusive scan over order of nchild
    int *posbase;        // [NC] new position of the first (frontmost) child of processed p
    int *newpos;         // [NC] new position of a surviving node p
    uint32_t *best;      // [NC]
};

int orb_octree_nc(const OrbParams &P)
{
    int nc = 0;
    for (int l = 0; l < P.nlevels; l++) { const int a = P.lv[l].quota + 16, b = 4 * P.lv[l].n_ini + 4; nc = a > nc ? a : nc; nc = b > nc ? b : nc; }
    return nc;
}

size_t orb_octree_lds_bytes(int nc)
{
    return (size_t)nc * 4 * (6 + 4 + 6) + 64;
}

__device__ __forceinline__ int oct_quadrant(uint32_t key, uint32_t b0, uint32_t b1)
{
    // DivideNode (ORBextractor.cc:479-524): halfX = ceil((UR.x-UL.x)/2), children by < on x then y
    const int x0 = b0 & 0xFFFF, y0 = b0 >> 16, x1 = b1 & 0xFFFF, y1 = b1 >> 16;
    const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
    const int kx = ORB_KEY_X(key), ky = ORB_KEY_Y(key);
    return (kx < mx ? 0 : 1) + (ky < my ? 0 : 2);          // n1=0 n2=1 n3=2 n4=3
}

#define OCT_KR 8               // candidates per thread held in registers (x 256 threads)
#ifdef OCT_PROF
__device__ long long g_oct_prof[8];           // debug build only (EXTRA=-DOCT_PROF): cycles of gather / roots / subdivision / best / output+perm of workgroup 0, passes
#define OCT_T(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const long long t_ = clock64(); g_oct_prof[i] += t_ - t_prev; t_prev = t_; } } while (0)
extern "C" int orbhip_debug_oct_prof(long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_oct_prof), 64) != hipSuccess) return -1;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_oct_prof), z, 64) != hipSuccess) return -1; }
    return 0;
}
#else
#define OCT_T(i) do { } while (0)
#endif
// Candidates of (frame, level) in reference order -- cells row-major, list order inside a cell -- into keys[]; the first OCT_KR * 256 of them also
// into the caller's registers rk[].  `smem` is scratch (cell offsets) until the final barrier.  Returns their number (same in every thread).
__device__ __forceinline__ int oct_gather(const OrbParams &P, const OrbLevel &L, int frame, int lvl, uint32_t *smem, int NC, int *wsum,
                                          uint32_t (&rk)[OCT_KR], uint32_t *keys)
{
    const int tid = threadIdx.x;
    // ---- gather candidates in reference order: cells row-major, list order inside a cell
    const uint32_t *ccount = P.cell_count + (size_t)frame * P.cells_per_frame + L.cell_base;
    const uint32_t *clist = P.cell_list + (size_t)frame * P.cell_list_frame_stride + (size_t)L.cell_base * L.cell_cap;
    const int ncells = L.ncols * L.nrows;
    int running = 0;
    if (ncells + 1 <= 16 * NC) {
        // cell offsets -> LDS (the node arrays are not in use yet), then ONE flat pass over the candidates: candidate k finds its cell by
        // binary search over the offsets and is fetched straight into its register slot (all loads of a thread independent and in
        // flight together; the per-cell copy loops this replaces were chains of dependent global round trips: 37 % of the kernel)
        int *coff = reinterpret_cast<int *>(smem);
        for (int c0 = 0; c0 < ncells; c0 += 256) {
            const int c = c0 + tid;
            const int n = c < ncells ? min((int)ccount[c], L.cell_cap) : 0;
            int total;
            const int off = running + block_excl_scan256(n, wsum, &total);
            if (c < ncells) coff[c] = off;
            running += total;
        }
        if (tid == 0) coff[ncells] = running;
        __syncthreads();
        if (running > L.key_cap) { if (tid == 0) atomicExch(P.status, ORBHIP_E_CAPACITY); running = L.key_cap; }
        const int K0 = running;
        auto fetch = [&](int k) {
            int lo = 0, hi = ncells;                                 // largest c with coff[c] <= k (empty cells share offsets: take the last)
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (coff[mid] <= k) lo = mid; else hi = mid; }
            return clist[(size_t)lo * L.cell_cap + (k - coff[lo])];
        };
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) { const int k = tid + 256 * i; rk[i] = k < K0 ? fetch(k) : 0u; }
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) { const int k = tid + 256 * i; if (k < K0) keys[k] = rk[i]; }
        for (int k = tid + 256 * OCT_KR; k < K0; k += 256) keys[k] = fetch(k);
        __syncthreads();                                         // coff is dead: the node arrays take the LDS over
    } else {
        for (int c0 = 0; c0 < ncells; c0 += 256) {
            const int c = c0 + tid;
            const int n = c < ncells ? (int)ccount[c] : 0;
            int total;
            const int off = running + block_excl_scan256(n, wsum, &total);
            for (int i = 0; i < n; i++)
                if (off + i < L.key_cap) keys[off + i] = clist[(size_t)c * L.cell_cap + i];
            running += total;
        }
        if (running > L.key_cap) { if (tid == 0) atomicExch(P.status, ORBHIP_E_CAPACITY); running = L.key_cap; }
        __syncthreads();                                     // keys[] visible block-wide (same CU, L1 coherent within WG)
        __threadfence_block();
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) { const int k = tid + 256 * i; rk[i] = k < running ? keys[k] : 0u; }
    }
    if (tid == 0) P.lvl_ncand[frame * P.nlevels + lvl] = running;
    return running;
}

// Best key of each of the `size` final nodes (rn[] / node_of[]: node of every candidate), the kept keys in list order and the spatial work order of
// k_orient_desc.  `best` = NC words of LDS.
__device__ __forceinline__ void oct_output(const OrbParams &P, const OrbLevel &L, int frame, int lvl, uint32_t *best, int size, int K,
                                           const uint32_t (&rk)[OCT_KR], const int (&rn)[OCT_KR], const uint32_t *keys, const uint16_t *node_of,
                                           long long &t_prev)
{
    const int tid = threadIdx.x;
    int32_t *count_out = P.lvl_count + frame * P.nlevels + lvl;
    // ---- best key per node: max response, first in list order wins (ORBextractor.cc:739-758)
    for (int i = tid; i < size; i += 256) best[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OCT_KR; i++)
        if (tid + 256 * i < K) atomicMax(&best[rn[i]], ((uint32_t)ORB_KEY_S(rk[i]) << 20) | (uint32_t)(0xFFFFF - (tid + 256 * i)));
    for (int k = tid + 256 * OCT_KR; k < K; k += 256)
        atomicMax(&best[node_of[k]], ((uint32_t)ORB_KEY_S(keys[k]) << 20) | (uint32_t)(0xFFFFF - k));
    __syncthreads();
    OCT_T(3);
    uint32_t *out = P.lvl_kp + (size_t)frame * P.kps_per_frame + L.kp_base;
    int nout = size;
    if (nout > L.kp_cap) { if (tid == 0) atomicExch(P.status, ORBHIP_E_CAPACITY); nout = L.kp_cap; }
    // processing order for k_orient_desc: rows of 32-pixel tiles, x inside a row (rank by counting over LDS; nout <= quota + 8)
    uint16_t *perm = P.lvl_perm + (size_t)frame * P.kps_per_frame + L.kp_base;
    uint32_t *wkey = P.lvl_wkey + (size_t)frame * P.kps_per_frame + L.kp_base;     // the keys in that order: the reader fetches key and position side by side
    for (int i = tid; i < nout; i += 256) out[i] = keys[0xFFFFF - (best[i] & 0xFFFFF)];
    if (P.batch < ORB_PERM_MIN_BATCH) { if (tid == 0) *count_out = nout; return; }     // few frames: cache reuse is not the limit, latency is
    __syncthreads();                                      // everyone has read best: it now holds the spatial sort keys
    for (int i = tid; i < nout; i += 256) { const uint32_t ki = out[i]; best[i] = ((uint32_t)(ORB_KEY_Y(ki) >> 5) << 16) | (uint32_t)ORB_KEY_X(ki); }
    __syncthreads();
    for (int i = tid; i < nout; i += 256) {
        const uint32_t si = best[i];
        int rank = 0;
        for (int j = 0; j < nout; j++) { const uint32_t sj = best[j]; rank += (sj < si) || (sj == si && j < i); }
        perm[rank] = (uint16_t)i;
        wkey[rank] = out[i];                               // this lane's own store of above
    }
    if (tid == 0) *count_out = nout;
    OCT_T(4);
}

__device__ __forceinline__ void oct_iterative(const OrbParams &P, const int lvl, const int frame)
{
    extern __shared__ uint32_t smem[];
    __shared__ int wsum[8];
    __shared__ int s_size, s_front, s_nexpand, s_rstar, s_T, s_nproc;
    const int tid = threadIdx.x;
    long long t_prev = 0;
#ifdef OCT_PROF
    t_prev = clock64();
#endif
    const OrbLevel &L = P.lv[lvl];
    const int N = L.quota;
    const int NC = P.oct_nc;
    // double-buffered node arrays (by list position): box0 = UL.x|UL.y<<16, box1 = BR.x|BR.y<<16, cnt = #keys
    uint32_t *box0 = smem, *box1 = smem + NC, *cnt = smem + 2 * NC;
    uint32_t *nbox0 = smem + 3 * NC, *nbox1 = smem + 4 * NC, *ncnt = smem + 5 * NC;
    OctLds S;
    {
        uint32_t *p = smem + 6 * NC;
        S.cc = p; p += 4 * NC;
        S.ord = (int *)p; p += NC; S.by_ord = (int *)p; p += NC; S.excl = (int *)p; p += NC;
        S.posbase = (int *)p; p += NC; S.newpos = (int *)p; p += NC; S.best = p; p += NC;
    }
    uint32_t *keys = P.keys + (size_t)frame * P.keys_per_frame + L.key_base;
    uint16_t *node_of = P.node_of + (size_t)frame * P.keys_per_frame + L.key_base;
    uint32_t rk[OCT_KR]; int rn[OCT_KR];
    int32_t *count_out = P.lvl_count + frame * P.nlevels + lvl;
    const int K = oct_gather(P, L, frame, lvl, smem, NC, wsum, rk, keys);
#pragma unroll
    for (int i = 0; i < OCT_KR; i++) rn[i] = 0;
    if (K == 0) { if (tid == 0) *count_out = 0; return; }
    // The first OCT_KR * 256 candidates (all of them unless a level holds more than 2048) live in REGISTERS from here on, key and
    // node id; candidates beyond that keep the global arrays.
    __syncthreads();
    __threadfence_block();
    OCT_T(0);
    // ---- roots (ORBextractor.cc:541-584)
    const int n_ini = L.n_ini;
    const int H = (L.h - ORB_MINB) - ORB_MINB;
    for (int i = tid; i < NC; i += 256) { cnt[i] = 0; ncnt[i] = 0; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OCT_KR; i++)
        if (tid + 256 * i < K) {
            const int r = (int)__fdiv_rn((float)ORB_KEY_X(rk[i]), L.hx);     // ORBextractor.cc:568
            rn[i] = r;
            atomicAdd(&ncnt[r], 1u);
        }
    for (int k = tid + 256 * OCT_KR; k < K; k += 256) {
        const int r = (int)__fdiv_rn((float)ORB_KEY_X(keys[k]), L.hx);
        node_of[k] = (uint16_t)r;
        atomicAdd(&ncnt[r], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        // compact non-empty roots, keep order; remap handled below through newpos
        int m = 0;
        for (int i = 0; i < n_ini; i++) {
            const uint32_t c = ncnt[i];
            S.newpos[i] = m;
            if (c) {
                box0[m] = (uint32_t)(int)__fmul_rn(L.hx, (float)i);              // UL.x | 0<<16
                box1[m] = (uint32_t)(int)__fmul_rn(L.hx, (float)(i + 1)) | ((uint32_t)H << 16);
                cnt[m] = c;
                m++;
            }
        }
        s_size = m; s_front = m;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OCT_KR; i++) if (tid + 256 * i < K) rn[i] = S.newpos[rn[i]];
    for (int k = tid + 256 * OCT_KR; k < K; k += 256) node_of[k] = (uint16_t)S.newpos[node_of[k]];
    __syncthreads();

    OCT_T(1);
    // ---- subdivision loop.  size / front are the same in every thread (derived from block-wide sums): kept in registers, no LDS broadcast
    bool final_phase = false;
    int size = s_size, front = s_front;
    for (int guard = 0; guard < 64; guard++) {
        // 1. candidate set + processing order
        int C;   // number of candidates
        if (!final_phase) {
            int run = 0;
            for (int p0 = 0; p0 < size; p0 += 256) {
                const int p = p0 + tid;
                const int f = (p < size && cnt[p] > 1) ? 1 : 0;
                int tot;
                const int o = run + block_excl_scan256(f, wsum, &tot);
                if (p < size) { S.ord[p] = f ? o : -1; if (f) S.by_ord[o] = p; }
                run += tot;
            }
            C = run;
        } else {
            // candidates: p < front with cnt > 1 ; order by (cnt desc, p asc)
            int run = 0;
            for (int p0 = 0; p0 < size; p0 += 256) {
                const int p = p0 + tid;
                const int f = (p < front && cnt[p] > 1) ? 1 : 0;
                int tot;
                const int o = run + block_excl_scan256(f, wsum, &tot);
                if (p < size) S.ord[p] = -1;
                if (f) S.excl[o] = p;                   // temp: compacted candidate list (ascending p)
                run += tot;
            }
            C = run;
            __syncthreads();
            for (int i = tid; i < C; i += 256) {
                const int p = S.excl[i];
                const uint32_t ci = cnt[p];
                int r = 0;
                for (int j = 0; j < C; j++) {
                    const uint32_t cj = cnt[S.excl[j]];
                    r += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
                }
                S.ord[p] = r;
                S.by_ord[r] = p;
            }
        }
        __syncthreads();
        if (C == 0) break;                               // size == prevSize -> bFinish
        // 2. child key counts of every candidate
        for (int i = tid; i < 4 * size; i += 256) S.cc[i] = 0;
        if (tid == 0) { s_nexpand = 0; s_rstar = C - 1; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < OCT_KR; i++)
            if (tid + 256 * i < K) {
                const int p = rn[i];
                if (S.ord[p] >= 0) atomicAdd(&S.cc[4 * p + oct_quadrant(rk[i], box0[p], box1[p])], 1u);
            }
        for (int k = tid + 256 * OCT_KR; k < K; k += 256) {
            const int p = node_of[k];
            if (S.ord[p] >= 0) atomicAdd(&S.cc[4 * p + oct_quadrant(keys[k], box0[p], box1[p])], 1u);
        }
        __syncthreads();
        // 3. exclusive scan over order of the non-empty-children counts
        {
            int run = 0;
            for (int o0 = 0; o0 < C; o0 += 256) {
                const int o = o0 + tid;
                int nch = 0;
                if (o < C) { const uint32_t *q = &S.cc[4 * S.by_ord[o]]; nch = (q[0] > 0) + (q[1] > 0) + (q[2] > 0) + (q[3] > 0); }
                int tot;
                const int e = run + block_excl_scan256(nch, wsum, &tot);
                if (o < C) {
                    S.excl[o] = e;
                    // final phase: stop after the first split that reaches N (ORBextractor.cc:727-728)
                    if (final_phase && size + e + nch - (o + 1) >= N) atomicMin(&s_rstar, o);
                }
                run += tot;
            }
        }
        __syncthreads();
        const int rstar = s_rstar;
        int T, nproc;
        {   // every thread reads the same LDS words: no single-thread phase, no barrier
            const uint32_t *q = &S.cc[4 * S.by_ord[rstar]];
            T = S.excl[rstar] + (q[0] > 0) + (q[1] > 0) + (q[2] > 0) + (q[3] > 0);
            nproc = rstar + 1;
        }
        // 4. positions of surviving nodes: T + rank among non-processed (old order)
        {
            int run = 0;
            for (int p0 = 0; p0 < size; p0 += 256) {
                const int p = p0 + tid;
                const int surv = (p < size && !(S.ord[p] >= 0 && S.ord[p] <= rstar)) ? 1 : 0;
                int tot;
                const int e = run + block_excl_scan256(surv, wsum, &tot);
                if (p < size && surv) S.newpos[p] = T + e;
                run += tot;
            }
        }
        // 5. build the new node arrays
        for (int p = tid; p < size; p += 256) {
            const int o = S.ord[p];
            if (o >= 0 && o <= rstar) {
                const uint32_t *q = &S.cc[4 * p];
                const int nch = (q[0] > 0) + (q[1] > 0) + (q[2] > 0) + (q[3] > 0);
                const int base = T - (S.excl[o] + nch);          // frontmost child (n4 side)
                S.posbase[p] = base;
                const uint32_t b0 = box0[p], b1 = box1[p];
                const int x0 = b0 & 0xFFFF, y0 = b0 >> 16, x1 = b1 & 0xFFFF, y1 = b1 >> 16;
                const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
                int pos = base, nexp = 0;
                for (int qd = 3; qd >= 0; qd--) {
                    if (q[qd]) {
                        const int cx0 = (qd & 1) ? mx : x0, cx1 = (qd & 1) ? x1 : mx;
                        const int cy0 = (qd & 2) ? my : y0, cy1 = (qd & 2) ? y1 : my;
                        nbox0[pos] = (uint32_t)cx0 | ((uint32_t)cy0 << 16);
                        nbox1[pos] = (uint32_t)cx1 | ((uint32_t)cy1 << 16);
                        ncnt[pos] = q[qd];
                        nexp += q[qd] > 1;
                        pos++;
                    }
                }
                if (nexp) atomicAdd(&s_nexpand, nexp);
            } else {
                const int np = S.newpos[p];
                nbox0[np] = box0[p]; nbox1[np] = box1[p]; ncnt[np] = cnt[p];
            }
        }
        __syncthreads();
        // 6. re-label keys
        auto relabel = [&](uint32_t key, int p) {
            const int o = S.ord[p];
            if (o >= 0 && o <= rstar) {
                const int qd = oct_quadrant(key, box0[p], box1[p]);
                const uint32_t *q = &S.cc[4 * p];
                int r = 0;                                         // non-empty siblings in front (q' > qd)
                for (int j = 3; j > qd; j--) r += q[j] > 0;
                return S.posbase[p] + r;
            }
            return S.newpos[p];
        };
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) if (tid + 256 * i < K) rn[i] = relabel(rk[i], rn[i]);
        for (int k = tid + 256 * OCT_KR; k < K; k += 256) node_of[k] = (uint16_t)relabel(keys[k], node_of[k]);
        __syncthreads();                                  // relabelled keys / new node arrays / s_nexpand complete; the next pass re-initialises s_nexpand
        const int new_size = T + (size - nproc);            // only after its own barrier (step 2), i.e. after every thread has read it here
        const int nexpand = s_nexpand;
        { uint32_t *t; t = box0; box0 = nbox0; nbox0 = t; t = box1; box1 = nbox1; nbox1 = t; t = cnt; cnt = ncnt; ncnt = t; }
        const int old_size = size;
        size = new_size; front = T;
#ifdef OCT_PROF
        if (blockIdx.x == 0 && tid == 0) g_oct_prof[5] += 1;
#endif
        // 7. termination (ORBextractor.cc:661-735)
        if (new_size >= N || new_size == old_size) break;
        if (!final_phase && new_size + 3 * nexpand > N) final_phase = true;
    }
    __syncthreads();
    OCT_T(2);
    oct_output(P, L, frame, lvl, S.best, size, K, rk, rn, keys, node_of, t_prev);
}

__global__ __launch_bounds__(256) void k_octree(OrbParams P)
{
    const int lvl = blockIdx.x / P.batch;              // level-major: big levels first
    oct_iterative(P, lvl, blockIdx.x - lvl * P.batch);
}

// ----------------------------------------------------------------------------------
// A5, table form: the same list without subdivision passes (model and derivation: tests/octree_table_model.py).
// A node's box follows from its root and its quadrant digits alone, and a full pass splits exactly the nodes the pass before it made.
// So every key computes its own path (root, digits to depth D) once, and per-depth COUNT TABLES indexed by path prefix -- counted
// at depth D, summed four children upward -- hold everything the loop decides from: the list size after pass t is the number of
// non-empty depth-t prefixes, nToExpand the number with more than one key.  The list after the last full pass T is generation T
// followed by the single-key nodes of generations T-1 .. 0; inside a generation list order is ascending path code once the digits
// at even distance from the last one (and the root, for odd t) are complemented -- push_front of n1..n4, parents reversed once more
// per pass.  The final phase works on that node list alone, its child counts are the next table.  In the end the tables are
// overwritten with list positions and every key looks its own path up.
// A list whose tree needs a table deeper than D leaves -1 in lvl_count; k_octree_redo runs the iterative form on those.
// ----------------------------------------------------------------------------------
#define OCT_DMAX_LIMIT 7
#define OCT_TAB_NODE_WORDS 9   // LDS words per node slot of the table form; the tables take the remaining 7 of orb_octree_lds_bytes()'s 16
__host__ __device__ __forceinline__ int oct_tab_off(int n_ini, int d) { return n_ini * (((1 << (2 * d)) - 1) / 3); }      // words of the tables of depths < d

int orb_octree_dmax(const OrbParams &P)
{
    int n_ini = 1;
    for (int l = 0; l < P.nlevels; l++) n_ini = P.lv[l].n_ini > n_ini ? P.lv[l].n_ini : n_ini;
    int d = 0;
    while (d < OCT_DMAX_LIMIT && (long)oct_tab_off(n_ini, d + 2) <= (long)(16 - OCT_TAB_NODE_WORDS) * P.oct_nc) d++;
    return d >= 2 ? d : 0;                                  // 0: no room for tables worth having -- the iterative form alone
}

__device__ __forceinline__ uint32_t oct_path(uint32_t key, const OrbLevel &L, int H, int D)
{
    const int kx = ORB_KEY_X(key), ky = ORB_KEY_Y(key);
    const int r = min((int)__fdiv_rn((float)kx, L.hx), L.n_ini - 1);                       // ORBextractor.cc:568
    int x0 = (int)__fmul_rn(L.hx, (float)r), x1 = (int)__fmul_rn(L.hx, (float)(r + 1)), y0 = 0, y1 = H;
    uint32_t path = (uint32_t)r;
    for (int d = 0; d < D; d++) {                                                         // DivideNode, as oct_quadrant
        const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
        const bool qx = kx >= mx, qy = ky >= my;
        x0 = qx ? mx : x0; x1 = qx ? x1 : mx; y0 = qy ? my : y0; y1 = qy ? y1 : my;
        path = (path << 2) | (uint32_t)((qx ? 1 : 0) + (qy ? 2 : 0));
    }
    return path;
}

__global__ __launch_bounds__(256) void k_octree_tab(OrbParams P)
{
    extern __shared__ uint32_t smem[];
    __shared__ int wsum[8];
    __shared__ int s_nz[OCT_DMAX_LIMIT + 1], s_mu[OCT_DMAX_LIMIT + 1];
    __shared__ int s_front, s_rstar;
    const int tid = threadIdx.x;
    long long t_prev = 0;
#ifdef OCT_PROF
    t_prev = clock64();
#endif
    const int lvl = blockIdx.x / P.batch;              // level-major: big levels first
    const int frame = blockIdx.x - lvl * P.batch;
    const OrbLevel &L = P.lv[lvl];
    const int N = L.quota, NC = P.oct_nc, D = P.oct_dmax, n_ini = L.n_ini;
    const int H = (L.h - ORB_MINB) - ORB_MINB;
    // node arrays by list position, double-buffered: cnt = #keys, tix = depth << 27 | path prefix
    uint32_t *cnt = smem, *ncnt = smem + NC, *tix = smem + 2 * NC, *ntix = smem + 3 * NC;
    int *ord = (int *)(smem + 4 * NC), *by_ord = (int *)(smem + 5 * NC), *excl = (int *)(smem + 6 * NC), *newpos = (int *)(smem + 7 * NC);
    uint32_t *best = smem + 8 * NC, *tab = smem + OCT_TAB_NODE_WORDS * NC;
    uint32_t *keys = P.keys + (size_t)frame * P.keys_per_frame + L.key_base;
    uint16_t *node_of = P.node_of + (size_t)frame * P.keys_per_frame + L.key_base;
    uint32_t rk[OCT_KR]; int rn[OCT_KR];
    int32_t *count_out = P.lvl_count + frame * P.nlevels + lvl;
    const int K = oct_gather(P, L, frame, lvl, smem, NC, wsum, rk, keys);
    if (K == 0) { if (tid == 0) *count_out = 0; return; }
    __syncthreads();
    OCT_T(0);
    // ---- 1. every key's path to depth D; counts at depth D (K atomics over n_ini * 4^D words, not over the few words of the shallow depths)
    {
        uint32_t *tabD = tab + oct_tab_off(n_ini, D);
        for (int i = tid; i < (n_ini << (2 * D)); i += 256) tabD[i] = 0;
        if (tid <= D) { s_nz[tid] = 0; s_mu[tid] = 0; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) {
            rn[i] = 0;
            if (tid + 256 * i < K) { const uint32_t p = oct_path(rk[i], L, H, D); rn[i] = (int)p; atomicAdd(&tabD[p], 1u); }
        }
        for (int k = tid + 256 * OCT_KR; k < K; k += 256) atomicAdd(&tabD[oct_path(keys[k], L, H, D)], 1u);
        __syncthreads();
    }
    // ---- 2. four children summed upward; per depth the number of non-empty prefixes and of those with more than one key
    for (int d = D; d >= 0; d--) {
        uint32_t *t = tab + oct_tab_off(n_ini, d);
        const uint32_t *c = tab + oct_tab_off(n_ini, d + 1);
        int tally = 0;                                                                        // non-empty | multi << 16 (a table has < 2^16 words)
        for (int i = tid; i < (n_ini << (2 * d)); i += 256) {
            uint32_t v;
            if (d < D) { v = c[4 * i] + c[4 * i + 1] + c[4 * i + 2] + c[4 * i + 3]; t[i] = v; } else v = t[i];
            tally += (v > 0 ? 1 : 0) + (v > 1 ? 0x10000 : 0);
        }
        tally = wave_sum_dpp(tally);
        if ((tid & (WAVE - 1)) == 0 && tally) { atomicAdd(&s_nz[d], tally & 0xFFFF); atomicAdd(&s_mu[d], tally >> 16); }
        __syncthreads();
    }
    OCT_T(1);
    // ---- 3. the last full pass T and whether the final phase follows (ORBextractor.cc:593-665); the same scalar logic in every thread
    int T = 0;
    bool final_phase = false;
    {
        int prev = s_nz[0];
        for (int t = 1; t <= D; t++) {
            const int sz = s_nz[t], nexpand = s_mu[t];
            if (sz >= N || sz == prev) { T = t; break; }                                     // includes the quirk: a pass that leaves the size unchanged ends the loop
            if (sz + 3 * nexpand > N) { T = t; final_phase = true; break; }
            if (nexpand == 0) { T = t; break; }                                              // nothing left to split: the next pass changes nothing
            prev = sz;
        }
    }
    if (T == 0) { if (tid == 0) *count_out = -1; return; }                                   // deeper than the tables: k_octree_redo
    // ---- 4. the node list after pass T: one scan over the entries of depths T, T-1, .. 0, each depth in its list order
    int size, front, dcur = T;
    {
        const int E = oct_tab_off(n_ini, T + 1), per = (E + 255) >> 8;
        const int e0 = min(tid * per, E), e1 = min(e0 + per, E);
        auto entry = [&](int e, uint32_t &c, uint32_t &tx) {
            int d = T, j = e;
            while (j >= (n_ini << (2 * d))) { j -= n_ini << (2 * d); d--; }
            const uint32_t m = (1u << (2 * d)) - 1;
            int root = j >> (2 * d);
            if (d & 1) root = n_ini - 1 - root;
            const uint32_t raw = ((uint32_t)root << (2 * d)) | (((uint32_t)j & m) ^ (0x33333333u & m));
            c = tab[oct_tab_off(n_ini, d) + raw];
            tx = ((uint32_t)d << 27) | raw;
            return c > 0 && (d == T || c == 1) && (d == 0 || tab[oct_tab_off(n_ini, d - 1) + (raw >> 2)] > 1);
        };
        uint32_t c, tx;
        int nf = 0;
        for (int e = e0; e < e1; e++) nf += entry(e, c, tx) ? 1 : 0;
        int pos = block_excl_scan256(nf, wsum, &size);
        if (size > NC) { if (tid == 0) *count_out = -1; return; }                             // (cannot happen: size <= max(N, 4 nIni); keeps the stores below in bounds)
        for (int e = e0; e < e1; e++) {
            if (e == (n_ini << (2 * T))) s_front = pos;                                       // generation T ends here
            if (entry(e, c, tx)) { cnt[pos] = c; tix[pos] = tx; pos++; }
        }
        __syncthreads();
        front = s_front;
    }
    // ---- 5. final phase on the nodes alone (ORBextractor.cc:671-735): as in the iterative form, child counts from the next table
    while (final_phase) {
        int C;
        {
            int run = 0;
            for (int p0 = 0; p0 < size; p0 += 256) {
                const int p = p0 + tid;
                const int f = (p < front && cnt[p] > 1) ? 1 : 0;
                int tot;
                const int o = run + block_excl_scan256(f, wsum, &tot);
                if (p < size) ord[p] = -1;
                if (f) excl[o] = p;                       // temp: compacted candidate list (ascending p)
                run += tot;
            }
            C = run;
        }
        __syncthreads();
        if (C == 0) break;                                // size == prevSize -> bFinish
        if (dcur == D) { if (tid == 0) *count_out = -1; return; }                           // the children's counts are below the tables
        for (int i = tid; i < C; i += 256) {              // order by (cnt desc, p asc)
            const int p = excl[i];
            const uint32_t ci = cnt[p];
            int r = 0;
            for (int j = 0; j < C; j++) {
                const uint32_t cj = cnt[excl[j]];
                r += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
            }
            ord[p] = r;
            by_ord[r] = p;
        }
        if (tid == 0) s_rstar = C - 1;
        __syncthreads();
        const uint32_t *ctab = tab + oct_tab_off(n_ini, dcur + 1);
        auto nchild = [&](int p) { const uint32_t *q = ctab + 4 * (tix[p] & 0x7FFFFFFu); return (q[0] > 0) + (q[1] > 0) + (q[2] > 0) + (q[3] > 0); };
        {
            int run = 0;
            for (int o0 = 0; o0 < C; o0 += 256) {
                const int o = o0 + tid;
                const int nch = o < C ? nchild(by_ord[o]) : 0;
                int tot;
                const int e = run + block_excl_scan256(nch, wsum, &tot);
                if (o < C) {
                    excl[o] = e;
                    if (size + e + nch - (o + 1) >= N) atomicMin(&s_rstar, o);              // stop after the first split that reaches N (ORBextractor.cc:727-728)
                }
                run += tot;
            }
        }
        __syncthreads();
        const int rstar = s_rstar;
        const int Tn = excl[rstar] + nchild(by_ord[rstar]), nproc = rstar + 1;
        {
            int run = 0;
            for (int p0 = 0; p0 < size; p0 += 256) {
                const int p = p0 + tid;
                const int surv = (p < size && !(ord[p] >= 0 && ord[p] <= rstar)) ? 1 : 0;
                int tot;
                const int e = run + block_excl_scan256(surv, wsum, &tot);
                if (p < size && surv) newpos[p] = Tn + e;
                run += tot;
            }
        }
        for (int p = tid; p < size; p += 256) {
            const int o = ord[p];
            if (o >= 0 && o <= rstar) {
                const uint32_t raw4 = 4 * (tix[p] & 0x7FFFFFFu);
                const uint32_t *q = ctab + raw4;
                int pos = Tn - (excl[o] + nchild(p));                                        // frontmost child (n4 side)
                for (int qd = 3; qd >= 0; qd--)
                    if (q[qd]) { ncnt[pos] = q[qd]; ntix[pos] = ((uint32_t)(dcur + 1) << 27) | (raw4 + qd); pos++; }
            } else {
                const int np = newpos[p];
                ncnt[np] = cnt[p]; ntix[np] = tix[p];
            }
        }
        __syncthreads();
        { uint32_t *t; t = cnt; cnt = ncnt; ncnt = t; t = tix; tix = ntix; ntix = t; }
        const int old_size = size;
        size = Tn + (size - nproc); front = Tn; dcur++;
#ifdef OCT_PROF
        if (blockIdx.x == 0 && tid == 0) g_oct_prof[5] += 1;
#endif
        if (size >= N || size == old_size) break;
    }
    // ---- 6. the tables become position tables; every key finds the one node of the list that lies on its path
    {
        const int Ef = oct_tab_off(n_ini, dcur + 1);
        for (int i = tid; i < Ef; i += 256) tab[i] = 0xFFFFFFFFu;
        __syncthreads();
        for (int p = tid; p < size; p += 256) { const uint32_t tx = tix[p]; tab[oct_tab_off(n_ini, (int)(tx >> 27)) + (tx & 0x7FFFFFFu)] = (uint32_t)p; }
        __syncthreads();
        auto node = [&](uint32_t path) {
            uint32_t nd = 0;
            for (int d = 0; d <= dcur; d++) { const uint32_t v = tab[oct_tab_off(n_ini, d) + (path >> (2 * (D - d)))]; if (v != 0xFFFFFFFFu) nd = v; }
            return (int)nd;
        };
#pragma unroll
        for (int i = 0; i < OCT_KR; i++) if (tid + 256 * i < K) rn[i] = node((uint32_t)rn[i]);
        for (int k = tid + 256 * OCT_KR; k < K; k += 256) node_of[k] = (uint16_t)node(oct_path(keys[k], L, H, D));
    }
    __syncthreads();
    OCT_T(2);
    oct_output(P, L, frame, lvl, best, size, K, rk, rn, keys, node_of, t_prev);
}

// The lists k_octree_tab left to the iterative form (lvl_count == -1): each workgroup looks at 64 (level, frame) pairs and runs those.
__global__ __launch_bounds__(256) void k_octree_redo(OrbParams P)
{
    __shared__ unsigned long long s_todo;
    const int tid = threadIdx.x, total = P.nlevels * P.batch, base = blockIdx.x * 64;
    if (tid < 64) {
        const int w = base + tid, lvl = w / P.batch;
        const bool f = w < total && P.lvl_count[(w - lvl * P.batch) * P.nlevels + lvl] < 0;
        const unsigned long long m = __ballot(f);
        if (tid == 0) s_todo = m;
    }
    __syncthreads();
    unsigned long long todo = s_todo;
    while (todo) {
        const int w = base + __ffsll((long long)todo) - 1, lvl = w / P.batch;
        todo &= todo - 1;
        oct_iterative(P, lvl, w - lvl * P.batch);
        __syncthreads();                                  // its LDS is reused by the next list
    }
}

const void *orb_octree_func(int which)
{
    return which == 0 ? reinterpret_cast<const void *>(k_octree) : which == 1 ? reinterpret_cast<const void *>(k_octree_tab) : reinterpret_cast<const void *>(k_octree_redo);
}

// oct_dmax > 0: the table form, then the iterative form on the lists it could not do (parts: 1 = the first launch only, 2 = the second only)
void orb_launch_octree(const OrbParams &P, hipStream_t s, int parts)
{
    const size_t lds = orb_octree_lds_bytes(P.oct_nc);      // > 64 KB from about 4000 features per level on: opted in by the caller
    const int lists = P.nlevels * P.batch;
    if (P.oct_dmax <= 0) { hipLaunchKernelGGL(k_octree, dim3(lists), dim3(256), lds, s, P); return; }
    if (parts & 1) hipLaunchKernelGGL(k_octree_tab, dim3(lists), dim3(256), lds, s, P);
    if (parts & 2) hipLaunchKernelGGL(k_octree_redo, dim3((lists + 63) / 64), dim3(256), lds, s, P);
}

// ----------------------------------------------------------------------------------
// A9  output assembly: level order, pt *= scale for level>0, lapping-area split
// (ORBextractor.cc:1104-1149).  One workgroup per frame.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assemble(OrbParams P)
{
    __shared__ int wsum[8];
    __shared__ int s_cnt[ORB_MAX_LEVELS + 1];
    const int tid = threadIdx.x, frame = blockIdx.x;
    if (tid == 0) {
        int n = 0;
        for (int l = 0; l < P.nlevels; l++) { s_cnt[l] = n; n += P.lvl_count[frame * P.nlevels + l]; }
        s_cnt[P.nlevels] = n;
    }
    __syncthreads();
    const int n = s_cnt[P.nlevels];
    orbhip_keypoint *okp = P.out_kp + (size_t)frame * P.max_kp;
    uint8_t *odesc = P.out_desc + (size_t)frame * P.max_kp * 32;
    int mono_run = 0;
    for (int g0 = 0; g0 < n; g0 += 256) {
        const int g = g0 + tid;
        int lvl = 0, stereo = 0;
        float fx = 0, fy = 0;
        size_t src = 0;
        if (g < n) {
            for (int l = 1; l < P.nlevels; l++) if (g >= s_cnt[l]) lvl = l;
            const OrbLevel &L = P.lv[lvl];
            src = (size_t)frame * P.kps_per_frame + L.kp_base + (g - s_cnt[lvl]);
            const uint32_t key = P.lvl_kp[src];
            fx = (float)(ORB_KEY_X(key) + ORB_MINB);
            fy = (float)(ORB_KEY_Y(key) + ORB_MINB);
            if (lvl != 0) { fx = __fmul_rn(fx, L.scale); fy = __fmul_rn(fy, L.scale); }    // :1131-1133
            stereo = (fx >= (float)P.lap0 && fx <= (float)P.lap1) ? 1 : 0;                 // :1135
        }
        int tot;
        const int mono_before = mono_run + block_excl_scan256((g < n && !stereo) ? 1 : 0, wsum, &tot);
        if (g < n) {
            const int stereo_before = g - mono_before;
            const int slot = stereo ? (n - 1 - stereo_before) : mono_before;
            const OrbLevel &L = P.lv[lvl];
            orbhip_keypoint kp;
            kp.x = fx; kp.y = fy; kp.size = L.size; kp.angle = P.lvl_angle[src];
            kp.response = (float)ORB_KEY_S(P.lvl_kp[src]);
            kp.octave = lvl; kp.class_id = -1;
            okp[slot] = kp;
            const uint4 *d = reinterpret_cast<const uint4 *>(P.lvl_desc + src * 32);
            uint4 *o = reinterpret_cast<uint4 *>(odesc + (size_t)slot * 32);
            o[0] = d[0]; o[1] = d[1];
        }
        mono_run += tot;
    }
    if (tid == 0) { P.out_count[frame] = n; P.out_mono[frame] = mono_run; }
}

void orb_launch_assemble(const OrbParams &P, hipStream_t s)
{
    hipLaunchKernelGGL(k_assemble, dim3(P.batch), dim3(256), 0, s, P);
}
