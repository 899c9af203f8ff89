// fast_kernels.hip -- the per-cell FAST stage of the ORB front-end: k_fast_cells (one wave per cell), k_fast_runs (opt-in: runs of
// two cells), the host plan of their parameter block and their launcher.
#include "orb_internal.h"
#include "wave_dpp.h"
#include <algorithm>
#include <mutex>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

// ----------------------------------------------------------------------------------
// A3/A4  per-cell FAST-9/16 + score + 3x3 NMS + two-threshold retry, ONE kernel, one wave per cell
// (ORBextractor.cc:783-854 calling cv::FAST twice; OpenCV FAST_t<16> / cornerScore<16>).
//
// Identity used (tests/test_oracle_orb.py::test_fast_arc_score_identity):
//   S = max over the 16 contiguous 9-arcs of min(v-p) and of min(p-v);
//   corner at threshold t  <=>  S > t ;  cornerScore == S-1.
// On RAW pixel values:  S = max(v - Hi, Lo - v),  Hi = min over arcs of (max of the arc's pixels), Lo = max over arcs of
// (min of the arc's pixels): the sixteen subtractions v - p disappear from the arc search.
//
// Per cell (one wave, no workgroup barriers): (1) the cell's sub-image (band + 3 px) is staged into LDS as packed u16
// PAIRS -- dword p of a row holds pixels (2p-1, 2p) relative to the sub-image, so a band pixel pair and its circle
// neighbours at even dx are plain dword reads and odd dx is one v_alignbit; (2) every band pixel pair runs the cheap
// necessary test ("a 9-arc contains one pixel of every diametral pair", 4 compass pairs, raw values) and is classified
// against BOTH thresholds; pairs that may hold a corner at iniThFAST go to an ordered queue; (3) the queue is scored
// densely (one pair per lane); (4) 3x3 strict NMS from an LDS score tile and ordered emission (cv::FAST order).  Only if
// the cell yields nothing at iniThFAST are the remaining candidates (minThFAST < M <= iniThFAST) scored and the NMS
// repeated at minThFAST (ORBextractor.cc:825-828).  NMS is threshold independent on raw scores: a corner at t survives
// iff score >= t and score > every neighbour's raw score, and a neighbour that is no corner at t has a smaller score
// anyway, so scores that were never computed count as 0.  No score map leaves the kernel.
// ----------------------------------------------------------------------------------
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));

__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ s16x2 pkmin(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ s16x2 pkmax(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
// Three-input packed min / max (round 4).  gfx950 has no v_pk_min3_i16, but v_pk_minimum3_f16 / v_pk_maximum3_f16 -- and a u16 pattern 0..255
// read as an f16 is the subnormal k x 2^-24 (f16 denormals are not flushed), whose order is the integers' order: for pixel values the two
// instructions ARE the integer min / max of three, exactly (all 2^24 triples checked on the device) and at the full rate (4.7 cycles per
// wave-instruction).  Only for operands known to be pixel values (never -1 / NaN patterns).
__device__ __forceinline__ s16x2 pkmin3(s16x2 a, s16x2 b, s16x2 c)
{
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(as_u32(a)), "v"(as_u32(b)), "v"(as_u32(c)));
    return as_s16x2(r);
}
__device__ __forceinline__ s16x2 pkmax3(s16x2 a, s16x2 b, s16x2 c)
{
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(as_u32(a)), "v"(as_u32(b)), "v"(as_u32(c)));
    return as_s16x2(r);
}
// pixel pair starting one pixel to the right of dword `lo`'s first pixel: (lo.hi, hi.lo)
__device__ __forceinline__ s16x2 pair_odd(uint32_t hi, uint32_t lo) { return as_s16x2(__builtin_amdgcn_alignbit(hi, lo, 16)); }

// Necessary-test value M of the band pixel pair whose centre dword is q[0] (q points into the pair tile, PITCH dwords per
// row): M = max(v - max_j min(a_j, b_j), min_j max(a_j, b_j) - v) over the 4 compass diametral pairs; S > t implies M > t.
template <int PITCH>
__device__ __forceinline__ s16x2 fc_compass(const uint32_t *q)
{
    const s16x2 v = as_s16x2(q[0]);
    const s16x2 n = as_s16x2(q[3 * PITCH]), s = as_s16x2(q[-3 * PITCH]);
    const s16x2 e = pair_odd(q[2], q[1]), w = pair_odd(q[-1], q[-2]);
    const s16x2 se = as_s16x2(q[2 * PITCH + 1]), nw = as_s16x2(q[-2 * PITCH - 1]);
    const s16x2 ne = as_s16x2(q[-2 * PITCH + 1]), sw = as_s16x2(q[2 * PITCH - 1]);
    const s16x2 lo = pkmax(pkmax3(pkmin(n, s), pkmin(e, w), pkmin(se, nw)), pkmin(ne, sw));
    const s16x2 hi = pkmin(pkmin3(pkmax(n, s), pkmax(e, w), pkmax(se, nw)), pkmax(ne, sw));
    return pkmax(v - lo, hi - v);
}

// Arc score S (threshold independent, packed) of the band pixel pair at q[0].  Circle in cv::makeOffsets order, k = 0..15:
// (0,3)(1,3)(2,2)(3,1)(3,0)(3,-1)(2,-2)(1,-3)(0,-3)(-1,-3)(-2,-2)(-3,-1)(-3,0)(-3,1)(-2,2)(-1,3)
template <int PITCH>
__device__ __forceinline__ s16x2 fc_arc_score(const uint32_t *q)
{
    s16x2 p[16];
    {
        const uint32_t *r = q + 3 * PITCH;                      // dy = +3: k = 15, 0, 1
        p[15] = pair_odd(r[0], r[-1]); p[0] = as_s16x2(r[0]); p[1] = pair_odd(r[1], r[0]);
        r = q + 2 * PITCH; p[14] = as_s16x2(r[-1]); p[2] = as_s16x2(r[1]);
        r = q + PITCH; p[13] = pair_odd(r[-1], r[-2]); p[3] = pair_odd(r[2], r[1]);
        p[12] = pair_odd(q[-1], q[-2]); p[4] = pair_odd(q[2], q[1]);
        r = q - PITCH; p[11] = pair_odd(r[-1], r[-2]); p[5] = pair_odd(r[2], r[1]);
        r = q - 2 * PITCH; p[10] = as_s16x2(r[-1]); p[6] = as_s16x2(r[1]);
        r = q - 3 * PITCH; p[9] = pair_odd(r[0], r[-1]); p[8] = as_s16x2(r[0]); p[7] = pair_odd(r[1], r[0]);
    }
    // The two 9-arcs starting at j-1 and at j (j odd) share the 8 pixels j..j+7:
    //   best of the two = combine(run8(j..j+7), better of the end pixels p[j-1], p[j+8])
    // so only the 8 odd-start 8-runs are needed (index m <-> j = 2m+1), built by doubling.
    s16x2 lo2[8], hi2[8], lo4[8], hi4[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { lo2[m] = pkmin(p[2 * m + 1], p[(2 * m + 2) & 15]); hi2[m] = pkmax(p[2 * m + 1], p[(2 * m + 2) & 15]); }
#pragma unroll
    for (int m = 0; m < 8; m++) { lo4[m] = pkmin(lo2[m], lo2[(m + 1) & 7]); hi4[m] = pkmax(hi2[m], hi2[(m + 1) & 7]); }
    // per odd start m: the darkest pixel of the better of its two 9-arcs / the brightest one (three-input forms: one instruction each)
    s16x2 xl[8], xh[8];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const s16x2 e0 = p[2 * m], e1 = p[(2 * m + 9) & 15];
        xl[m] = pkmin3(lo4[m], lo4[(m + 2) & 7], pkmax(e0, e1));
        xh[m] = pkmax3(hi4[m], hi4[(m + 2) & 7], pkmin(e0, e1));
    }
    // Lo = brightest "darkest pixel of an arc", Hi = darkest "brightest pixel of an arc"
    const s16x2 Lo = pkmax(pkmax3(pkmax3(xl[0], xl[1], xl[2]), xl[3], xl[4]), pkmax3(xl[5], xl[6], xl[7]));
    const s16x2 Hi = pkmin(pkmin3(pkmin3(xh[0], xh[1], xh[2]), xh[3], xh[4]), pkmin3(xh[5], xh[6], xh[7]));
    const s16x2 v = as_s16x2(q[0]);
    return pkmax(v - Hi, Lo - v);
}

#define FC_ID(by, bp) (((by) << 5) | (bp))      // band pixel pair id: row | pair (pairs per row <= 32)
#define FC_U(v) as_s16x2(__builtin_amdgcn_perm(0u, (uint32_t)(v), 0x0c010c00u))      // a score-tile entry, left | right << 8  ->  packed halves
// ---- what k_fast_cells and k_fast_runs share word for word, as macros expanded in place (the rule of desc_kernels.hip); they use the
// kernels' names lane, ld, dh, PT, SC, PITCH, SPITCH
// (1) stage: the NLD_ chunks this lane loaded (fc_issue_loads, NCH_ chunks per row) go to the pair tile, PT[r][p] = pixels (ini_x + 2p - 1,
// ini_x + 2p) of sub-image row r as u16 | u16 << 16; the score tile starts at zero (guards included): a pair that is never scored
// counts as 0 in the NMS
#define FC_STAGE(NCH_, NLD_) do { \
        const int last = (dh + 6) * NCH_ - 1; \
        _Pragma("unroll") \
        for (int t = 0; t < NLD_; t++) { \
            const int i = min(lane + 64 * t, last); \
            const int r = (int)(__umul24((uint32_t)i, 65536u / NCH_ + 1) >> 16), c = i - r * NCH_; \
            uint4 a, b; \
            a.x = __builtin_amdgcn_perm(0u, ld[t].x, 0x0c010c00u); a.y = __builtin_amdgcn_perm(0u, ld[t].x, 0x0c030c02u); \
            a.z = __builtin_amdgcn_perm(0u, ld[t].y, 0x0c010c00u); a.w = __builtin_amdgcn_perm(0u, ld[t].y, 0x0c030c02u); \
            b.x = __builtin_amdgcn_perm(0u, ld[t].z, 0x0c010c00u); b.y = __builtin_amdgcn_perm(0u, ld[t].z, 0x0c030c02u); \
            b.z = __builtin_amdgcn_perm(0u, ld[t].w, 0x0c010c00u); b.w = __builtin_amdgcn_perm(0u, ld[t].w, 0x0c030c02u); \
            uint4 *dst = reinterpret_cast<uint4 *>(&PT[r * PITCH + 8 * c]); \
            dst[0] = a; dst[1] = b; \
        } \
        uint4 *scz = reinterpret_cast<uint4 *>(SC); \
        for (int i = lane; i < ((dh + 2) * SPITCH + 7) / 8; i += 64) scz[i] = make_uint4(0u, 0u, 0u, 0u); \
    } while (0)
// (4) the 3x3 neighbourhood of the pair at score-tile entry q: sc = its own entry; declares V = above / below each pixel, Lc (.y: the column
// left of the pair, three rows), Rc (.x: the column right of it)
#define FC_NMS_NEIGHBOURS() \
    sc = q[0]; \
    const s16x2 V = pkmax(FC_U(q[-SPITCH]), FC_U(q[SPITCH])); \
    const s16x2 Lc = pkmax3(FC_U(q[-SPITCH - 1]), FC_U(q[-1]), FC_U(q[SPITCH - 1])); \
    const s16x2 Rc = pkmax3(FC_U(q[-SPITCH + 1]), FC_U(q[1]), FC_U(q[SPITCH + 1]))

// What the staging loads of a cell need, in SGPRs: band height, image row pitch, pixel (ini_x - 1, ini_y) of the level image (first byte staged)
struct FcSrc { int dh, ipitch; const uint8_t *src; };
#define FC_SGPR(x) __builtin_amdgcn_readfirstlane(x)
// A cell's record: one scalar 16-byte load (the table is written by reserve and never by a kernel: the constant address space lets the
// compiler use the scalar cache although the kernel stores to global memory)
typedef uint32_t fc_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) fc_u32x4 *fc_tab_ptr;
__device__ __forceinline__ FcRecord fc_load_record(const FcRecord *tab, int i)
{
    const fc_u32x4 v = ((fc_tab_ptr)(uintptr_t)tab)[i];
    return FcRecord{v.x, v.y, v.z, v.w};
}
// The cell of record R in frame `frame`: one small load of the level's image by level, one multiply-add for the pixel
__device__ __forceinline__ FcSrc fc_cell_src(const FastParams &P, const FcRecord &R, int frame)
{
    const FcImage &I = P.im[fc_rec_level(R)];
    const int ipitch = I.pitch & 0xFFFF;
    return FcSrc{fc_rec_dh(R), ipitch, I.img + (size_t)(uint32_t)frame * I.frame_stride + (uint32_t)(fc_rec_y0(R) * ipitch + fc_rec_x0(R))};
}
// Staging loads of a cell: its sub-image rows as NCH 16-byte chunks each (chunk c = pixels ini_x - 1 + 16c .. + 15 = pairs 8c .. 8c+7),
// flattened (row, chunk) tasks, NLD per lane, branch-free (surplus lanes repeat the last task), all in flight together.  A chunk may
// run past the sub-image: those bytes are never used and lie inside the frame (the sub-image ends >= 16 rows above the image's end).
template <int NCH, int NLD, typename CELL>
__device__ __forceinline__ void fc_issue_loads(const CELL &C, int lane, uint4 (&ld)[NLD])
{
    const int last = max((C.dh + 6) * NCH - 1, 0);
#pragma unroll
    for (int t = 0; t < NLD; t++) {
        const int i = min(lane + 64 * t, last);
        const int r = (int)(__umul24((uint32_t)i, 65536u / NCH + 1) >> 16), c = i - r * NCH;      // i / NCH for i < 1024
        const u32x4_unaligned v = *reinterpret_cast<const u32x4_unaligned *>(C.src + (uint32_t)(__umul24((uint32_t)r, (uint32_t)C.ipitch) + 16u * (uint32_t)c));
        ld[t] = make_uint4(v.x, v.y, v.z, v.w);
    }
}

#ifdef FC_PROF
// debug build only (make EXTRA=-DFC_PROF): wave-cycles of k_fast_cells by phase, summed over all waves -- stage (load wait, LDS writes, next cell's
// record and loads) / sync / necessary test / arc scores / NMS + emission / tail; [6] cells, [7] whole kernel; [8] LDS writes of the stage,
// [9] wait for / decode of the next cell's record, [10] issue of its loads (the three parts of [0], which is then only the rest)
__device__ unsigned long long g_fc_prof[12];
extern "C" int orbhip_debug_fc_prof(unsigned long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_fc_prof), 96) != hipSuccess) return -1;
    if (reset) { unsigned long long z[12] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_fc_prof), z, 96) != hipSuccess) return -1; }
    return 0;
}
// (the sums live in LDS, 96 bytes per wave of the debug build only: twelve 64-bit sums in scalar registers cost the cell loop hundreds of spills)
#define FC_T(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); if (lane == 0) fc_acc[i] += t_ - fc_prev; fc_prev = t_; } while (0)
#else
#define FC_T(i) do { } while (0)
#endif
// One wave per workgroup, persistent over chunks of consecutive cells (frame-major, then level, then row-major): the next
// cell's staging loads are in flight while the current cell is processed.  LDS (private to the wave, no barriers): pair tile
// PT [rows][PITCH = 8 NCH], score tile SC [srows + 2][SPITCH] (one guard row / pair all around), queue Q.
// The wave holds a position (frame, record index) and nothing else of the geometry: a cell's numbers come from its record of the cell
// table (orb_plan_fast), whose load goes out a cell ahead, at the top of the cell before.
template <int NCH, int SPITCH, int NLD>
__global__ __launch_bounds__(64) void k_fast_cells(FastParams P)
{
    constexpr int PITCH = 8 * NCH;
    extern __shared__ __attribute__((aligned(16))) uint32_t fc_lds[];
    const int lane = threadIdx.x;
    uint32_t *PT = fc_lds;
    uint16_t *SC = reinterpret_cast<uint16_t *>(PT + P.rows * PITCH);          // scores, one u16 per pixel pair: left | right << 8 (cornerScore <= 254)
    uint16_t *Q = SC + (P.srows + 2) * SPITCH;
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    // Work is dealt in CHUNKS of consecutive cells, chunk c to wave c mod #waves: cells differ a lot in cost (texture, clipped border cells,
    // the small top levels), and contiguous equal-count ranges per wave left the kernel waiting for its slowest waves -- its time did not
    // move between 8 and 21 waves per CU.  Neighbouring chunks still run on neighbouring waves of one XCD (shared aprons hit its L2).
    // The cells of levels [lvl_lo, lvl_hi) are records [cell_lo, cell_hi) of a frame; cell number g of the launch (32 bits: the launcher
    // refuses more) is record cell_lo + g % cps of frame g / cps.
    const uint32_t chunk = (uint32_t)FC_SGPR(P.chunk), ncells = FC_SGPR(P.total);
    uint32_t g = FC_SGPR(lid * chunk);                                 // current cell (a wave beyond the last chunk leaves)
    if (g >= ncells) return;
    const int cell_lo = FC_SGPR(P.cell_lo), cell_hi = FC_SGPR(P.cell_hi), cps = cell_hi - cell_lo;
    const int ini_th = FC_SGPR(P.ini_th), min_th = FC_SGPR(P.min_th), cpf = FC_SGPR(P.cells_per_frame);
    int frame = FC_SGPR((int)(g / (uint32_t)cps));                      // the only division: once per wave
    int ti = cell_lo + (int)(g - (uint32_t)frame * (uint32_t)cps);      // current record
    uint32_t left = min(chunk, ncells - g) - 1;                          // cells of the current chunk after this one
    FcRecord R = fc_load_record(P.cell_tab, ti);
    uint4 ld[NLD];
    fc_issue_loads<NCH, NLD>(fc_cell_src(P, R, frame), lane, ld);
    const int lo_th = min(ini_th, min_th);
#ifdef FC_PROF
    __shared__ unsigned long long fc_acc[12];
    if (lane < 12) fc_acc[lane] = 0;
    unsigned long long fc_prev = __builtin_readcyclecounter();
    const unsigned long long fc_t0 = fc_prev;
#endif
    for (bool more = true; more;) {
        // ---- next cell: the next one of the chunk, or (hop cells on) the first one of this wave's next chunk.  Its record is asked for now and
        // read after the stage
        const bool inside = left > 0;
        const uint32_t gn = g + (inside ? 1u : FC_SGPR(P.hop));
        more = gn < ncells;
        int nframe = frame + (inside ? 0 : (int)FC_SGPR(P.hop_q)), nti = ti + (inside ? 1 : (int)FC_SGPR(P.hop_r));
        if (nti >= cell_hi) { nti -= cps; nframe++; }
        const FcRecord N = fc_load_record(P.cell_tab, more ? nti : ti);
        left = inside ? left - 1 : min(chunk, ncells - gn) - 1;         // (unused when there is no next cell)
        const int dw = fc_rec_dw(R), dh = fc_rec_dh(R);
        const int npb = (dw + 1) >> 1;                             // band pixel pairs per row
        uint32_t *cnt_out = P.cell_count + (uint32_t)(frame * cpf + ti);
        uint32_t *list = P.cell_list + ((size_t)(uint32_t)frame * P.cell_list_frame_stride + R.list);
        const uint32_t key0 = fc_rec_key0(R);                      // packed key of band pixel (0, 0): x and y of a band pixel add without a carry (12 bits each)
        const int cell_cap = FC_SGPR(P.cell_cap), tpr = fc_rec_tpr(R), rptT = fc_rec_rpt(R);
        const uint32_t magic = fc_rec_magic(R);
#ifdef FC_PROF
        __builtin_amdgcn_s_waitcnt(0x0F70);                       // vmcnt(0): the wait for this cell's staging loads on its own counter
        FC_T(11);
#endif
        // ---- (1) stage: PT[r][p] = pixels (ini_x + 2p - 1, ini_x + 2p) of sub-image row r as u16 | u16 << 16
        if (dw > 0) FC_STAGE(NCH, NLD);
        FC_T(8);
        // ---- the next cell's loads stay in flight while this one is processed
        const FcSrc NS = fc_cell_src(P, N, nframe);
        FC_T(9);
        if (more) fc_issue_loads<NCH, NLD>(NS, lane, ld);
        FC_T(10);
        if (dw <= 0) { if (lane == 0) *cnt_out = 0; R = N; g = gn; frame = nframe; ti = nti; continue; }
        FC_T(0);
        wave_lds_sync();           // (also: the previous cell's LDS reads are done before this cell's writes -- same wave, program order)
        // Lane layout of the necessary test from the level's nominal cell width (clipped border cells leave lanes idle): tasks per row tpr,
        // rows per trip rpt, two adjacent pairs per lane
        const int tr0 = (int)(__umul24((uint32_t)lane, magic) >> 16), tg = lane - tr0 * tpr;
        const bool lane_rows = tr0 < rptT && 2 * tg < npb, pair1 = 2 * tg + 1 < npb;
        int total = 0;
        FC_T(1);
        for (int pass = 0; pass < 2; pass++) {
            // ---- (2) necessary test on every band pixel pair at this pass's threshold, rows in order (queue order = cv::FAST order).  No
            // per-pair state is kept: the rare second pass (nothing at iniThFAST, ORBextractor.cc:825-828) runs the test again at minThFAST
            // and scores everything it lets through (the pairs of the first pass among them: same scores again)
            const int th = pass == 0 ? ini_th : min_th;
            const s16x2 thP = (s16x2){(short)(th + 1), (short)(th + 1)};
            int nq1 = 0;                                               // entries of Q (wave-uniform)
            for (int y0 = 0; y0 < dh; y0 += rptT) {
                const int by = y0 + tr0;
                bool f0 = false, f1 = false;                           // pair 0 / 1 may hold a corner at th
                if (lane_rows && by < dh) {
                    const uint32_t *q = &PT[(by + 3) * PITCH + 2 * tg + 2];
                    // M - (th + 1) >= 0 in a half <=> its sign bit is clear (|M| <= 255: no overflow).  An odd band's last lane evaluates one pair
                    // beyond the band: its flag is dropped here
                    const uint32_t SIGN = 0x80008000u;
                    const s16x2 M0 = fc_compass<PITCH>(q), M1 = fc_compass<PITCH>(q + 1);      // straight-line: the LDS reads of both pairs go out together
                    f0 = (as_u32(M0 - thP) & SIGN) != SIGN;
                    f1 = ((as_u32(M1 - thP) & SIGN) != SIGN) & pair1;
                }
                const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1);      // (outside the branch: the counts below must stay wave-uniform)
                const int pos = nq1 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                                (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
                if (f0) Q[pos] = (uint16_t)FC_ID(by, 2 * tg);
                if (f1) Q[pos + (f0 ? 1 : 0)] = (uint16_t)FC_ID(by, 2 * tg + 1);
                nq1 += __popcll(b0) + __popcll(b1);
            }
            wave_lds_sync();
            FC_T(2);
            // ---- (3) dense arc score, one pair per lane
            for (int i0 = 0; i0 < nq1; i0 += 64) {
                const int i = min(i0 + lane, nq1 - 1);
                const int id = Q[i], by = id >> 5, bp = id & 31;
                const s16x2 S = fc_arc_score<PITCH>(&PT[(by + 3) * PITCH + bp + 2]);
                if (i0 + lane < nq1) {
                    const uint32_t lo = S.x > lo_th ? (uint32_t)(S.x - 1) : 0u;
                    const uint32_t hi = (S.y > lo_th && 2 * bp + 1 < dw) ? (uint32_t)(S.y - 1) : 0u;
                    SC[(by + 1) * SPITCH + bp + 1] = (uint16_t)(lo | (hi << 8));
                }
            }
            wave_lds_sync();
            FC_T(3);
            // ---- (4) 3x3 strict NMS on raw scores + threshold gate + ordered emission.  The two pixels of a pair are neighbours and the NMS
            // is strict, so at most one of them is kept: a lane emits 0 or 1 corner, and its rank among the 64 entries is a ballot's count of
            // the lanes below it, not a prefix sum over the wave
            for (int i0 = 0; i0 < nq1; i0 += 64) {
                const int i = i0 + lane;
                uint32_t keep = 0, sc = 0;
                int by = 0, bp = 0;
                if (i < nq1) {
                    const int id = Q[i];
                    by = id >> 5; bp = id & 31;
                    const uint16_t *q = &SC[(by + 1) * SPITCH + bp + 1];
                    FC_NMS_NEIGHBOURS();
                    const int sl = (int)(sc & 0xFFu), sr = (int)(sc >> 8);
                    const int nbl = max(max((int)V.x, (int)V.y), max((int)Lc.y, sr));                // L: above, below, the R column (3 rows), left column
                    const int nbr = max(max((int)V.x, (int)V.y), max((int)Rc.x, sl));
                    if (sl >= th && sl > nbl) keep = 1u;                   // (sl > nbl >= sr and sr > nbr >= sl exclude each other)
                    if (sr >= th && sr > nbr) keep = 2u;
                }
                const unsigned long long kb = __builtin_amdgcn_ballot_w64(keep != 0);
                const int offs = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(kb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kb, 0u));
                if (keep != 0 && offs < cell_cap)
                    list[offs] = (keep & 1u ? ORB_PACK_KEY(2 * bp, by, sc & 0xFFu) : ORB_PACK_KEY(2 * bp + 1, by, sc >> 8)) + key0;
                total += __popcll(kb);
            }
            FC_T(4);
            if (total > 0 || min_th == ini_th) break;              // vKeysCell not empty at iniThFAST: done
            wave_lds_sync();                                        // the second pass rewrites Q and SC
        }
        if (total > cell_cap) { if (lane == 0) atomicExch(P.status, ORBHIP_E_CAPACITY); total = cell_cap; }
        if (lane == 0) *cnt_out = (uint32_t)total;
        R = N; g = gn; frame = nframe; ti = nti;
        FC_T(5);
#ifdef FC_PROF
        if (lane == 0) fc_acc[6]++;
#endif
    }
#ifdef FC_PROF
    if (lane == 0) fc_acc[7] = __builtin_readcyclecounter() - fc_t0;
    wave_lds_sync();
    if (lane < 12) atomicAdd(&g_fc_prof[lane], fc_acc[lane]);
#endif
}

// ----------------------------------------------------------------------------------
// k_fast_runs (round 4): the same per-cell FAST semantics (ORBextractor.cc:783-854: every cell is FASTed alone at
// iniThFAST, again at minThFAST iff that left it empty; the 3-px ring of its sub-image is excluded, so NMS never sees a neighbour cell)
// with the cell no longer the unit of work.  A wave owns a RUN of up to two horizontally adjacent cells of one cell row -- one
// sub-image of (2 wCell + 6) x (hCell + 6) pixels, staged once (80-byte rows instead of two 41..48-byte ones: less apron, longer lines)
// -- and the cell enters only as
//   (a) a mask in the NMS: a neighbour pixel that lies in the other cell's band counts as 0,
//   (b) the per-cell "empty at iniThFAST -> again at minThFAST" decision (the second pass is restricted to the pixels of empty cells),
//   (c) the emission: per-cell ranks by ballot, per-cell lists and counts.
// The necessary (compass) test, which is most of the kernel, no longer gathers its 11 dwords per pixel pair from LDS: lane = pair COLUMN
// (32 columns x 2 half waves, the halves walking the upper / lower half of the rows), and a lane walks DOWN its column with a
// register ring of the last seven rows' three dwords (columns c-1, c, c+1), so a row step costs 3 LDS instructions (the new row's
// ds_read2 + ds_read, the centre row's two outer dwords) instead of 11 and no address arithmetic; the loop is unrolled by the ring
// period so that every ring access is a fixed register.  Queue (two, one per half wave: concatenated they are in cv::FAST's raster
// order), dense arc scoring and the score tile are k_fast_cells' -- the very same expressions, so every candidate list comes out
// byte-identical (tests/test_gpu_orb.py compares them with the oracle cell by cell).
// ----------------------------------------------------------------------------------
#define FR_PITCH 40            // pair-tile dwords per row: pairs -2 .. 37 of the run's sub-image
#define FR_SPITCH 40           // score-tile u16 per row: 32 pairs + one guard on either side
#define FR_NCH 5               // 16-byte chunks staged per row
struct FrRun {
    int frame, lvl, ci, cj, nc;         // first cell of the run, cells in it (1 or 2)
    int dw0, dw1, dh;                   // detection band widths of the two cells (0: the reference skips the cell), band height
    int ipitch; const uint8_t *src;     // pixel (ini_x - 1, ini_y) of the first cell: first byte staged
    int ncols, nrows, wcell, hcell, cell_base, cell_cap, rpc, rpr;
};
__device__ __forceinline__ void fr_run_geom(const FastParams &P, FrRun &C)
{
    const FcLevel &L = P.lv[C.lvl];
    C.ncols = FC_SGPR(L.ncols); C.nrows = FC_SGPR(L.nrows); C.wcell = FC_SGPR(L.wcell); C.hcell = FC_SGPR(L.hcell);
    C.cell_base = FC_SGPR(L.cell_base); C.cell_cap = FC_SGPR(L.cell_cap); C.rpc = FC_SGPR(L.rpc); C.rpr = FC_SGPR(L.rpr);
    const FcImage &I = P.im[C.lvl];
    C.ipitch = FC_SGPR(I.pitch) & 0xFFFF;
    C.nc = min(C.rpc, C.ncols - C.cj);
    const int max_bx = FC_SGPR(L.max_bx), max_by = FC_SGPR(L.max_by);
    const int ini_y = ORB_MINB + C.ci * C.hcell, ini_x = ORB_MINB + C.cj * C.wcell;
    C.src = I.img + (size_t)C.frame * I.frame_stride + (size_t)(ini_y * C.ipitch + ini_x - 1);
    C.dw0 = 0; C.dw1 = 0; C.dh = 0;
    if (ini_y >= max_by - 3) return;                                          // ORBextractor.cc:788
    C.dh = min(ini_y + C.hcell + 6, max_by) - ini_y - 6;
    if (C.dh <= 0) { C.dh = 0; return; }
    if (ini_x < max_bx - 6) C.dw0 = max(min(ini_x + C.wcell + 6, max_bx) - ini_x - 6, 0);     // :797-802
    const int ini_x1 = ini_x + C.wcell;
    if (C.nc > 1 && ini_x1 < max_bx - 6) C.dw1 = max(min(ini_x1 + C.wcell + 6, max_bx) - ini_x1 - 6, 0);
    if (C.dw0 == 0) C.dw1 = 0;
}

// FR_NLD: staging loads per lane (rows x 5 chunks <= 64 FR_NLD): 4 for cells of up to 45 rows, 6 up to 70
template <int FR_NLD>
__global__ __launch_bounds__(64) void k_fast_runs(FastParams P)
{
    constexpr int PITCH = FR_PITCH, SPITCH = FR_SPITCH;
    extern __shared__ __attribute__((aligned(16))) uint32_t fc_lds[];
    const int lane = threadIdx.x;
    uint32_t *PT = fc_lds;
    uint16_t *SC = reinterpret_cast<uint16_t *>(PT + P.run_rows * PITCH);      // scores, one u16 per pixel pair: left | right << 8
    uint16_t *Q = SC + (P.srows + 2) * SPITCH;                                  // [0, q0): upper half of the rows, [q0, ..): lower half
    const int q0cap = FC_SGPR(P.run_q0);
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    const int lvl_lo = FC_SGPR(P.lvl_lo), lvl_hi = FC_SGPR(P.lvl_hi);
    const int run_lo = FC_SGPR(P.lv[lvl_lo].run_base);
    const int rps = (lvl_hi < P.nlevels ? FC_SGPR(P.lv[lvl_hi].run_base) : FC_SGPR(P.runs_per_frame)) - run_lo;
    const long total_runs = (long)P.batch * rps;
    const int chunk = FC_SGPR(P.chunk);
    const long nchunks = (total_runs + chunk - 1) / chunk;
    if ((long)lid >= nchunks) return;
    const int nlevels = lvl_hi, ini_th = FC_SGPR(P.ini_th), min_th = FC_SGPR(P.min_th), cpf = FC_SGPR(P.cells_per_frame);
    auto decode = [&](long gi, FrRun &X) {
        X.frame = (int)(gi / rps);
        const int run = run_lo + (int)(gi - (long)X.frame * rps);
        X.lvl = lvl_lo;
        for (int l = lvl_lo + 1; l < nlevels; l++) if (run >= P.lv[l].run_base) X.lvl = l;
        const int r = run - P.lv[X.lvl].run_base;
        X.ci = r / P.lv[X.lvl].rpr; X.cj = (r - X.ci * P.lv[X.lvl].rpr) * P.lv[X.lvl].rpc;
        X.frame = FC_SGPR(X.frame); X.lvl = FC_SGPR(X.lvl); X.ci = FC_SGPR(X.ci); X.cj = FC_SGPR(X.cj);
        fr_run_geom(P, X);
    };
    long ch = lid;
    long g = ch * chunk, g_end = min(g + chunk, total_runs);
    FrRun C;
    decode(g, C);
    uint4 ld[FR_NLD];
    fc_issue_loads<FR_NCH, FR_NLD>(C, lane, ld);
    const int lo_th = min(ini_th, min_th);
    const int bp = lane & 31, half = lane >> 5;                                // this lane's pair column and half wave
    for (bool more = true; more;) {
        const int dw0 = C.dw0, dw1 = C.dw1, dw = dw0 + dw1, dh = C.dh;
        const int npb = (dw + 1) >> 1;                             // band pixel pairs per row of the run
        const int cell = C.cell_base + C.ci * C.ncols + C.cj;
        uint32_t *cnt_out = P.cell_count + (size_t)C.frame * cpf + cell;
        uint32_t *list = P.cell_list + (size_t)C.frame * P.cell_list_frame_stride + (size_t)cell * C.cell_cap;
        const int key_x0 = 3 + C.cj * C.wcell, key_y0 = 3 + C.ci * C.hcell;
        const int cell_cap = C.cell_cap, nc = C.nc;
        // ---- (1) stage: PT[r][p] = pixels (ini_x + 2p - 1, ini_x + 2p) of sub-image row r as u16 | u16 << 16
        if (dw > 0) FC_STAGE(FR_NCH, FR_NLD);
        // ---- next run: its loads stay in flight while this one is processed
        FrRun N = C;
        g++;
        if (g < g_end) {
            N.cj += C.rpc;
            if (N.cj >= C.ncols) { N.cj = 0; N.ci++; }
            if (N.ci == C.nrows) { N.ci = 0; N.lvl++; }
            if (N.lvl == nlevels) { N.lvl = lvl_lo; N.frame++; }
            fr_run_geom(P, N);
        } else {
            ch += gridDim.x;
            more = ch < nchunks;
            if (more) { g = ch * chunk; g_end = min(g + chunk, total_runs); decode(g, N); }
        }
        if (more) fc_issue_loads<FR_NCH, FR_NLD>(N, lane, ld);
        if (dw <= 0) { if (lane < nc) cnt_out[lane] = 0; C = N; continue; }
        wave_lds_sync();
        // the cell of a band pixel: x < dw0 -> the first one.  B = first column of the second cell (or beyond every pixel)
        const int B = dw1 > 0 ? dw0 : (1 << 20);
        const int hh = (dh + 1) >> 1;                               // rows per half wave
        const int rb = half * hh;                                   // first band row of this lane's half
        const int rows_mine = min(hh, dh - rb);                     // (may be < hh for the lower half of an odd band)
        int tot0 = 0, tot1 = 0;                                     // keypoints emitted per cell (uniform)
        uint32_t empty = 0;                                         // second pass: bit c = cell c came out empty at iniThFAST
        for (int pass = 0; pass < 2; pass++) {
            const int th = pass == 0 ? ini_th : min_th;
            const s16x2 thP = (s16x2){(short)(th + 1), (short)(th + 1)};
            // a pair takes part if it lies in the band and, in the second pass, if one of its pixels belongs to an empty cell
            bool col_on = bp < npb;
            if (pass) col_on = col_on && ((((2 * bp >= B) ? 2u : 1u) | ((2 * bp + 1 >= B) ? 2u : 1u)) & empty) != 0;
            // ---- (2) necessary test, every lane walking down its pair column, seven rows per trip: the 13 tile rows a trip touches sit in
            // registers (six carried over from the previous trip), the seven M values are computed as seven independent chains (the
            // packed 16-bit min / max ops need a wait state between dependent ones: alone, a chain was half s_nop), then flagged and queued
            int nq0 = 0, nq1 = 0;
            {
                const uint32_t *col = PT + rb * PITCH + bp + 1;     // dwords [0], [1], [2] of a row = columns c - 1, c, c + 1 (c = bp + 2)
                const int rows_on = col_on ? rows_mine : 0;         // rows of this lane that may flag
                uint32_t rm[13], rc[13], rp[13];
#pragma unroll
                for (int i = 0; i < 6; i++) { rm[i] = col[i * PITCH]; rc[i] = col[i * PITCH + 1]; rp[i] = col[i * PITCH + 2]; }
                const uint32_t SIGN = 0x80008000u;
                for (int y0 = 0; y0 < hh; y0 += 7) {
                    const uint32_t *cy = col + y0 * PITCH;
                    uint32_t cm2[7], cp2[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) {                   // (rows past the band: inside the tile's padding, never flagged)
                        rm[6 + i] = cy[(6 + i) * PITCH]; rc[6 + i] = cy[(6 + i) * PITCH + 1]; rp[6 + i] = cy[(6 + i) * PITCH + 2];
                        cm2[i] = cy[(3 + i) * PITCH - 1]; cp2[i] = cy[(3 + i) * PITCH + 3];
                    }
                    bool f[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        // fc_compass with q[0] = rc[i + 3]: n = q[3 P], s = q[-3 P], e = (q[1], q[2]), w = (q[-2], q[-1]), se = q[2 P + 1],
                        // nw = q[-2 P - 1], ne = q[-2 P + 1], sw = q[2 P - 1]
                        const s16x2 v = as_s16x2(rc[i + 3]);
                        const s16x2 n = as_s16x2(rc[i + 6]), so = as_s16x2(rc[i]);
                        const s16x2 e = pair_odd(cp2[i], rp[i + 3]), w = pair_odd(rm[i + 3], cm2[i]);
                        const s16x2 se = as_s16x2(rp[i + 5]), nw = as_s16x2(rm[i + 1]);
                        const s16x2 ne = as_s16x2(rp[i + 1]), sw = as_s16x2(rm[i + 5]);
                        const s16x2 lo = pkmax(pkmax3(pkmin(n, so), pkmin(e, w), pkmin(se, nw)), pkmin(ne, sw));
                        const s16x2 hi = pkmin(pkmin3(pkmax(n, so), pkmax(e, w), pkmax(se, nw)), pkmax(ne, sw));
                        const s16x2 M = pkmax(v - lo, hi - v);
                        f[i] = y0 + i < rows_on && (as_u32(M - thP) & SIGN) != SIGN;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        const unsigned long long b = __ballot(f[i]);
                        const uint32_t blo = (uint32_t)b, bhi = (uint32_t)(b >> 32);
                        // entries of the upper half go to Q[nq0 ..), of the lower half to Q[q0cap + nq1 ..): one expression for both
                        const int m = (int)__builtin_amdgcn_mbcnt_hi(bhi, __builtin_amdgcn_mbcnt_lo(blo, 0u));
                        const int pos = m + (half ? q0cap + nq1 - __popc(blo) : nq0);
                        if (f[i]) Q[pos] = (uint16_t)FC_ID(rb + y0 + i, bp);
                        nq0 += __popc(blo); nq1 += __popc(bhi);
                    }
#pragma unroll
                    for (int i = 0; i < 6; i++) { rm[i] = rm[7 + i]; rc[i] = rc[7 + i]; rp[i] = rp[7 + i]; }
                }
            }
            const int nq = nq0 + nq1;
            wave_lds_sync();
            // ---- (3) dense arc score, one pair per lane (queue entry i: the upper half's entries first)
            for (int i0 = 0; i0 < nq; i0 += 64) {
                const int i = min(i0 + lane, nq - 1);
                const int id = Q[i < nq0 ? i : q0cap + i - nq0], by = id >> 5, qp = id & 31;
                const s16x2 S = fc_arc_score<PITCH>(&PT[(by + 3) * PITCH + qp + 2]);
                if (i0 + lane < nq) {
                    const uint32_t lo = S.x > lo_th ? (uint32_t)(S.x - 1) : 0u;
                    const uint32_t hi = (S.y > lo_th && 2 * qp + 1 < dw) ? (uint32_t)(S.y - 1) : 0u;
                    SC[(by + 1) * SPITCH + qp + 1] = (uint16_t)(lo | (hi << 8));
                }
            }
            wave_lds_sync();
            // ---- (4) 3x3 strict NMS on raw scores (neighbours in the other cell's band count as 0) + threshold gate + per-cell ordered emission
            for (int i0 = 0; i0 < nq; i0 += 64) {
                const int i = i0 + lane;
                uint32_t keep = 0, sc = 0;
                int by = 0, qp = 0;
                if (i < nq) {
                    const int id = Q[i < nq0 ? i : q0cap + i - nq0];
                    by = id >> 5; qp = id & 31;
                    const uint16_t *q = &SC[(by + 1) * SPITCH + qp + 1];
                    FC_NMS_NEIGHBOURS();
                    const int xl = 2 * qp, xr = xl + 1;
                    const int sl = (int)(sc & 0xFFu), sr = (int)(sc >> 8);
                    // L: above / below, the column to its left (not if L is the second cell's first column), the R column (not across the boundary)
                    const int nbl = max(max((int)V.x, xl != B ? (int)Lc.y : 0), xr != B ? max((int)V.y, sr) : 0);
                    const int nbr = max(max((int)V.y, xr + 1 != B ? (int)Rc.x : 0), xr != B ? max((int)V.x, sl) : 0);
                    const bool onL = !pass || ((xl >= B ? 2u : 1u) & empty), onR = !pass || ((xr >= B ? 2u : 1u) & empty);
                    if (sl >= th && sl > nbl && onL) keep |= 1u;
                    if (sr >= th && sr > nbr && onR) keep |= 2u;
                }
                const int xl = 2 * qp;
                const bool kL = keep & 1u, kR = keep & 2u, cL = xl >= B, cR = xl + 1 >= B;      // kept flags, cell (0 / 1) of each pixel
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const bool mL = kL && (int)cL == c, mR = kR && (int)cR == c;
                    const unsigned long long bL = __ballot(mL), bR = __ballot(mR);
                    const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bL >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bL, 0u)) +
                                       (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bR >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bR, 0u));
                    const int base = c ? tot1 : tot0;
                    uint32_t *lst = list + (size_t)c * cell_cap;
                    if (mL) { const int o = base + before; if (o < cell_cap) lst[o] = ORB_PACK_KEY(xl + key_x0, by + key_y0, sc & 0xFFu); }
                    if (mR) { const int o = base + before + (mL ? 1 : 0); if (o < cell_cap) lst[o] = ORB_PACK_KEY(xl + 1 + key_x0, by + key_y0, (sc >> 8) & 0xFFu); }
                    const int add = __popcll(bL) + __popcll(bR);
                    if (c) tot1 += add; else tot0 += add;
                }
            }
            if (pass || min_th == ini_th) break;
            empty = (tot0 == 0 && dw0 > 0 ? 1u : 0u) | (tot1 == 0 && dw1 > 0 ? 2u : 0u);        // vKeysCell.empty() at iniThFAST (ORBextractor.cc:825-828)
            if (!empty) break;
            wave_lds_sync();                                        // the second pass rewrites Q and SC
        }
        if (tot0 > cell_cap || tot1 > cell_cap) { if (lane == 0) atomicExch(P.status, ORBHIP_E_CAPACITY); tot0 = min(tot0, cell_cap); tot1 = min(tot1, cell_cap); }
        if (lane == 0) { cnt_out[0] = (uint32_t)tot0; if (nc > 1) cnt_out[1] = (uint32_t)tot1; }
        C = N;
    }
}
const void *orb_fast_runs_func(int nld) { return nld == 4 ? reinterpret_cast<const void *>(k_fast_runs<4>) : reinterpret_cast<const void *>(k_fast_runs<6>); }

// staging loads per lane of k_fast_runs (its template argument), and the instance the launch below takes: 0 / 1 = k_fast_cells for large /
// small cells, 2 / 3 = k_fast_runs<4> / <6>
int orb_fast_runs_nld(const FastParams &F) { return (F.run_rows - 7) * FR_NCH <= 256 ? 4 : 6; }
int orb_fast_variant(const FastParams &F) { return F.use_runs ? (orb_fast_runs_nld(F) == 4 ? 2 : 3) : F.small_cells ? 1 : 0; }
// The FAST cell grid of a level from its size (ORBextractor.cc:771-781); false: the level is smaller than one cell
bool orb_plan_cell_grid(OrbLevel &L)
{
    const float w_ = (float)((L.w - ORB_EDGE + 3) - ORB_MINB), h_ = (float)((L.h - ORB_EDGE + 3) - ORB_MINB);
    if (w_ < 30.f || h_ < 30.f) return false;
    L.ncols = (int)(w_ / 30.f); L.nrows = (int)(h_ / 30.f);
    L.wcell = (int)ceilf(w_ / L.ncols); L.hcell = (int)ceilf(h_ / L.nrows);
    return true;
}
// Host plan (no HIP call): the kernels' compact parameter block from the extractor's geometry -- k_fast_cells' cell table (one record
// per cell of a frame, FcRecord), per level the cell grid for k_fast_runs, per-wave LDS geometry from the largest cell of this
// extractor.  Image pointers, batch and outputs are set per call.
void orb_plan_fast(const OrbParams &P, FastParams &F, std::vector<FcRecord> &cell_tab)
{
    memset(&F, 0, sizeof(F));
    cell_tab.clear(); cell_tab.reserve((size_t)P.cells_per_frame);
    for (int l = 0; l < P.nlevels; l++) {
        const OrbLevel &L = P.lv[l];
        const int max_bx = L.w - ORB_MINB, max_by = L.h - ORB_MINB;
        const int npb = (L.wcell + 1) >> 1;                            // band pixel pairs per row of a full cell
        const uint32_t tpr = (uint32_t)((npb + 1) >> 1), magic = 65536u / tpr + 1;     // two adjacent pairs per lane
        for (int ci = 0; ci < L.nrows; ci++)
            for (int cj = 0; cj < L.ncols; cj++) {
                const int ini_y = ORB_MINB + ci * L.hcell, ini_x = ORB_MINB + cj * L.wcell;
                int dw = 0, dh = 0;
                if (!(ini_y >= max_by - 3 || ini_x >= max_bx - 6)) {          // ORBextractor.cc:788,797
                    dw = std::min(ini_x + L.wcell + 6, max_bx) - ini_x - 6; dh = std::min(ini_y + L.hcell + 6, max_by) - ini_y - 6;
                    if (dw <= 0 || dh <= 0) dw = dh = 0;
                }
                FcRecord r;
                r.xy = (uint32_t)(ini_x - 1) | (uint32_t)ini_y << 16;
                r.band = (uint32_t)dw | (uint32_t)dh << 6 | tpr << 12 | magic << 16;
                r.key = ORB_PACK_KEY(3 + cj * L.wcell, 3 + ci * L.hcell, l);
                r.list = (uint32_t)(L.cell_base + ci * L.ncols + cj) * (uint32_t)L.cell_cap;
                cell_tab.push_back(r);
            }
    }
    F.cell_cap = P.lv[0].cell_cap;
    int mw = 0, mh = 0;
    bool small = true;
    for (int l = 0; l < P.nlevels; l++) {
        const OrbLevel &L = P.lv[l];
        FcLevel &f = F.lv[l];
        mw = std::max(mw, L.wcell); mh = std::max(mh, L.hcell);
        f.max_bx = L.w - ORB_MINB; f.max_by = L.h - ORB_MINB;
        f.ncols = L.ncols; f.nrows = L.nrows; f.wcell = L.wcell; f.hcell = L.hcell; f.cell_base = L.cell_base; f.cell_cap = L.cell_cap;
        const int npb = (L.wcell + 1) >> 1;                            // band pixel pairs per row
        small = small && npb + 4 <= 24 && npb + 2 <= 24 && (L.hcell + 6) * 3 <= 64 * 2;       // <3, 24, 2>: 24 pairs per row, 128 chunk tasks
    }
    {   // k_fast_runs: a wave works on a RUN of cells of one cell row -- two while both fit the 32 pixel-pair columns of a half wave
        int runs = 0;
        bool ok = true;
        for (int l = 0; l < P.nlevels; l++) {
            const OrbLevel &L = P.lv[l];
            FcLevel &f = F.lv[l];
            f.rpc = 2 * L.wcell <= 64 ? 2 : 1;
            f.rpr = (L.ncols + f.rpc - 1) / f.rpc;
            f.run_base = runs; runs += f.rpr * L.nrows;
            ok = ok && L.wcell <= 64 && L.hcell + 6 <= 70 && L.wcell >= 8 && L.hcell >= 8;
        }
        const int hh = (mh + 1) / 2;
        F.runs_per_frame = runs;
        F.run_rows = mh + 6 + 7;                                               // + the rows a seven-row trip of the column walk may read past the band
        F.run_q0 = (hh * 32 + 7) & ~7;                                         // first queue: the upper half of the rows (u16 entries)
        F.run_dw = F.run_rows * FR_PITCH + (((mh + 2) * FR_SPITCH + 2 * F.run_q0) + 1) / 2;   // pair tile + u16 score tile + u16 queues
        F.run_dw = (F.run_dw + 3) & ~3;
        // OPT-IN (ORBHIP_FAST_KERNEL=runs when the extractor reserves): bit-exact (tests/test_gpu_fast_cases.py runs every crafted case with it), but measured
        // SLOWER than k_fast_cells -- 1.72 ms (row-at-a-time ring) / 2.43 ms (seven-row trips) against 1.49 ms per 1024 VGA frames
        F.use_runs = ok && getenv("ORBHIP_FAST_KERNEL") && !strcmp(getenv("ORBHIP_FAST_KERNEL"), "runs") ? 1 : 0;
    }
    const int npb = (mw + 1) >> 1;
    F.small_cells = small ? 1 : 0;
    F.rows = mh + 6; F.srows = mh; F.qcap = (mh * npb + 1) & ~1;
    F.wave_dw = F.rows * (small ? 24 : 40) + ((F.srows + 2) * (small ? 24 : 32) + F.qcap + 1) / 2;      // pair tile (dwords) + u16 score tile + u16 queue
    F.wave_dw = (F.wave_dw + 3) & ~3;
    F.nlevels = P.nlevels; F.ini_th = P.ini_th; F.min_th = P.min_th; F.cells_per_frame = P.cells_per_frame;
}
// The plan's cell table, decoded, for per-level image sizes w[l] x h[l] (host only, no HIP call; tests/test_fast_cell_table.py).  out: 12
// ints per cell -- level, x0, y0 (first staged pixel), dw, dh, key_x0, key_y0, list offset, tpr, rpt, magic, cell_cap; at most cap cells
// are written.  Returns the cells of a frame, or a negative error (a level smaller than one cell, or a cell larger than the LDS tile).
extern "C" int orbhip_fast_cell_table(int nlevels, const int *w, const int *h, int *out, int cap)
{
    if (nlevels < 1 || nlevels > ORB_MAX_LEVELS || !w || !h || (!out && cap > 0)) return ORBHIP_E_BADARG;
    OrbParams P;
    memset(&P, 0, sizeof(P));
    P.nlevels = nlevels;
    int cells = 0, cell_cap = 0;
    for (int l = 0; l < nlevels; l++) {
        OrbLevel &L = P.lv[l];
        L.w = w[l]; L.h = h[l];
        if (!orb_plan_cell_grid(L) || L.wcell + 6 > 64 || L.hcell + 6 > 64) return ORBHIP_E_BADARG;
        cell_cap = std::max(cell_cap, ((L.wcell + 1) / 2) * ((L.hcell + 1) / 2));
        L.cell_base = cells; cells += L.ncols * L.nrows;
    }
    for (int l = 0; l < nlevels; l++) P.lv[l].cell_cap = cell_cap;
    P.cells_per_frame = cells;
    FastParams F;
    std::vector<FcRecord> tab;
    orb_plan_fast(P, F, tab);
    for (int i = 0; i < cells && i < cap; i++) {
        const FcRecord &r = tab[i];
        const uint32_t k = fc_rec_key0(r);
        const int v[12] = {fc_rec_level(r), fc_rec_x0(r), fc_rec_y0(r), fc_rec_dw(r), fc_rec_dh(r), ORB_KEY_X(k), ORB_KEY_Y(k), (int)r.list,
                           fc_rec_tpr(r), fc_rec_rpt(r), (int)fc_rec_magic(r), F.cell_cap};
        memcpy(out + 12 * i, v, sizeof(v));
    }
    return cells;
}

bool orb_launch_fast_cells(const FastParams &F_, hipStream_t s, int max_per_cu, int lvl_lo, int lvl_hi)
{
    FastParams F = F_;
    F.lvl_lo = lvl_lo; F.lvl_hi = lvl_hi < 0 ? F.nlevels : lvl_hi;
    if (F.lvl_lo >= F.lvl_hi) return true;
    const bool runs = F.use_runs != 0;
    // persistent single-wave workgroups: as many as the LDS lets a CU hold, a whole number per XCD
    const size_t lds = sizeof(uint32_t) * (size_t)(runs ? F.run_dw : F.wave_dw);
    // as many as the runtime says fit (LDS, wave slots), asked once per (device, kernel variant, LDS size).  The left and right images
    // of a stereo frame are extracted on two threads (Frame.cc:109-110) and a process may drive several GPUs: the table is guarded
    const int nld = orb_fast_runs_nld(F);
    const int v = orb_fast_variant(F);
    int per_cu;
    {
        struct Occ { int dev, v, n; size_t lds; };
        static std::mutex occ_mu; static std::vector<Occ> occ_tab;
        int dev = 0; (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> g(occ_mu);
        const Occ *hit = nullptr;
        for (const Occ &o : occ_tab) if (o.dev == dev && o.v == v && o.lds == lds) { hit = &o; break; }
        if (!hit) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, v >= 2 ? orb_fast_runs_func(nld) : orb_fast_cells_func(v), 64, lds) != hipSuccess || n < 1) n = (int)((160 * 1024) / (lds + 512));
            occ_tab.push_back(Occ{dev, v, n < 1 ? 1 : n, lds}); hit = &occ_tab.back();
            if (getenv("ORBHIP_DEBUG_FAST")) fprintf(stderr, "[orbhip] %s: %zu B of LDS per wave, %d waves per CU resident\n", v >= 2 ? "k_fast_runs" : "k_fast_cells", lds, hit->n);
        }
        per_cu = hit->n;
    }
    if (max_per_cu > 0 && per_cu > max_per_cu) per_cu = max_per_cu;      // leave LDS and wave slots to a kernel running beside this one
    long nblocks = (long)(F.n_cus > 0 ? F.n_cus : 256) * per_cu;
    const long total = runs ? (long)F.batch * ((F.lvl_hi < F.nlevels ? F.lv[F.lvl_hi].run_base : F.runs_per_frame) - F.lv[F.lvl_lo].run_base)
                            : (long)F.batch * ((F.lvl_hi < F.nlevels ? F.lv[F.lvl_hi].cell_base : F.cells_per_frame) - F.lv[F.lvl_lo].cell_base);
    if (nblocks > total) nblocks = (total + 7) / 8 * 8;
    // chunks of up to 4 consecutive cells (8 runs): they share aprons and level parameters; at least ~8 chunks per wave so that the shares even out.
    // (Round 4: 16 -> 4 cells.  The waves of an XCD work on neighbouring chunks at the same time, so the seam and apron lines of the k-th cells
    // of neighbouring chunks are touched together, but the last cell of one chunk and the first of the next 15 cell times (~0.1 ms) apart --
    // long after the line left the 4 MB L2.  1024 VGA frames: step 3.59 -> 3.55 ms at 4, 3.68 at 32; 1 and 2 lose to the per-chunk decode.)
    static const int chunk_env = getenv("ORBHIP_TUNE_FAST_CHUNK") ? atoi(getenv("ORBHIP_TUNE_FAST_CHUNK")) : 0;
    const long fair = total / (8 * nblocks);
    const int cmax = runs ? 8 : 4;
    F.chunk = chunk_env > 0 ? std::min(chunk_env, 1 << 16) : (int)(fair < 1 ? 1 : fair > cmax ? cmax : fair);
    if (!runs) {
        // k_fast_cells counts cells in 32 bits (no 64-bit division per chunk): the launch's cells, and one hop beyond the last, must fit
        const long hop = nblocks * F.chunk - F.chunk + 1;              // from the last cell of a chunk to the first cell of the wave's next chunk
        if (total + nblocks * (long)F.chunk >= (1l << 32) || (long)F.batch * F.cells_per_frame >= (1l << 31)) return false;
        F.cell_lo = F.lv[F.lvl_lo].cell_base; F.cell_hi = F.lvl_hi < F.nlevels ? F.lv[F.lvl_hi].cell_base : F.cells_per_frame;
        const long cps = F.cell_hi - F.cell_lo;
        F.total = (uint32_t)total; F.hop = (uint32_t)hop; F.hop_q = (uint32_t)(hop / cps); F.hop_r = (uint32_t)(hop % cps);
    }
    if (runs && nld == 4) hipLaunchKernelGGL(k_fast_runs<4>, dim3((unsigned)nblocks), dim3(64), lds, s, F);
    else if (runs) hipLaunchKernelGGL(k_fast_runs<6>, dim3((unsigned)nblocks), dim3(64), lds, s, F);
    else if (F.small_cells) hipLaunchKernelGGL((k_fast_cells<3, 24, 2>), dim3((unsigned)nblocks), dim3(64), lds, s, F);
    else hipLaunchKernelGGL((k_fast_cells<5, 32, 5>), dim3((unsigned)nblocks), dim3(64), lds, s, F);
    return true;
}
const void *orb_fast_cells_func(int small) { return small ? reinterpret_cast<const void *>(k_fast_cells<3, 24, 2>) : reinterpret_cast<const void *>(k_fast_cells<5, 32, 5>); }

