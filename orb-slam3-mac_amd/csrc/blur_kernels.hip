// blur_kernels.hip -- the blurred pyramid of the ORB front-end: k_blur (LDS tiles), k_blur_rows (row streaming), k_blur_mfma (matrix
// cores; this object alone is built with -mllvm -amdgpu-mfma-vgpr-form), the rule that picks one by batch size, their host plan and launcher.
#include "orb_internal.h"
#include "wave_dpp.h"
#include <cstdlib>

// ----------------------------------------------------------------------------------
// A7  7x7 sigma-2 Gaussian, 8-bit fixed point, BORDER_REFLECT_101 (ORBextractor.cc:1114-1115;
// arithmetic SURVEY Appendix A.7).  Separable inside LDS: the row pass of an 8-bit image
// with the q8 kernel (sum 257) fits u16 exactly (255*257 = 65535), column pass
// (sum + 2^15) >> 16 saturated.  Tile: 64x32 outputs per 256-thread workgroup.
// ----------------------------------------------------------------------------------
#define BL_TW 64
#define BL_TH 32
#define BL_ROWS (BL_TH + 6)
#define BL_IPD 20             // staged-row pitch (dwords): 3 pad | left apron | 16 tile dwords; the right apron is dword 0 of the next row
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (p < 0) p = -p;
    if (p >= n) p = 2 * n - 2 - p;
    return p;
}

// four pixels x..x+3 of an image row with BORDER_REFLECT_101 outside [0, w)  (x % 4 == 0)
__device__ __forceinline__ uint32_t bl_load4(const uint8_t *row, int x, int w)
{
    if (x >= 0 && x + 3 < w) return *reinterpret_cast<const uint32_t *>(row + x);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int xx = reflect101(x + j, w);
        xx = min(max(xx, 0), w - 1);
        v |= (uint32_t)row[xx] << (8 * j);
    }
    return v;
}

// horizontal 7-tap of four neighbouring pixels from the 12-byte window d0|d1|d2 (pixel 0 = byte 4), u16 each
__device__ __forceinline__ void bl_row4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t klo, uint32_t khi, uint32_t (&o)[4])
{
    o[0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0, 1), klo, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d2, d1, 1), khi, 0u, false), false);
    o[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0, 2), klo, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d2, d1, 2), khi, 0u, false), false);
    o[2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0, 3), klo, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d2, d1, 3), khi, 0u, false), false);
    o[3] = __builtin_amdgcn_udot4(d1, klo, __builtin_amdgcn_udot4(d2, khi, 0u, false), false);
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bl_dot2(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), c, false);
}

// ----------------------------------------------------------------------------------
// A7 over every pyramid level in ONE launch: the 64x32 tile (+3 rows / +4 columns of apron, BORDER_REFLECT_101) is staged
// with one 16-byte load per lane; row pass on v_dot4_u32_u8 (two rows per task, u16 sums written vertically PAIRED),
// column pass on v_dot2_u32_u16 (a 7-tap column = four dot2), saturate + pack, dword stores.
// Bound by vector-instruction issue (~19 lane-ops per pixel).  Algorithmic bytes: S read + S written.
// ----------------------------------------------------------------------------------
// tile cursor of a persistent k_blur workgroup: (level, frame, tile row / column), advanced without divisions
struct BlTile { int level, frame, tx, ty, ntx, nty, w, h, pitch; const uint8_t *src; uint8_t *dst; int dpitch; };
__device__ __forceinline__ void bl_tile_level(const OrbParams &P, BlTile &T)
{
    const OrbLevel &L = P.lv[T.level];
    T.w = __builtin_amdgcn_readfirstlane(L.w); T.h = __builtin_amdgcn_readfirstlane(L.h);
    T.pitch = __builtin_amdgcn_readfirstlane(L.img_pitch); T.dpitch = __builtin_amdgcn_readfirstlane(L.blur_pitch);
    T.ntx = (T.w + BL_TW - 1) / BL_TW; T.nty = (T.h + BL_TH - 1) / BL_TH;
}
__device__ __forceinline__ void bl_tile_frame(const OrbParams &P, BlTile &T)
{
    const OrbLevel &L = P.lv[T.level];
    T.src = L.img + (size_t)T.frame * L.img_frame_stride; T.dst = L.blur + (size_t)T.frame * L.blur_frame_stride;
}
// this lane's share of a tile's staging: lanes 0..151 one 16-byte chunk (38 rows x 4), lanes 152..227 one apron dword
__device__ __forceinline__ uint4 bl_stage_load(const BlTile &T, int tid)
{
    const bool chunk = tid < 4 * BL_ROWS;
    const int a = tid - 4 * BL_ROWS;
    const int r = chunk ? tid >> 2 : a >> 1;
    const int x0 = T.tx * BL_TW, y0 = T.ty * BL_TH, w = T.w;
    int y = reflect101(y0 + r - 3, T.h);
    y = min(max(y, 0), T.h - 1);
    const uint8_t *row = T.src + (uint32_t)__umul24((uint32_t)y, (uint32_t)T.pitch);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (chunk) {
        const int x = x0 + 16 * (tid & 3);
        if (x + 15 < w) v = *reinterpret_cast<const uint4 *>(row + x);
        else { v.x = bl_load4(row, x, w); v.y = bl_load4(row, x + 4, w); v.z = bl_load4(row, x + 8, w); v.w = bl_load4(row, x + 12, w); }
    } else if (a < 2 * BL_ROWS) {
        v.x = bl_load4(row, (a & 1) ? x0 + BL_TW : x0 - 4, w);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_blur(OrbParams P)
{
    __shared__ __attribute__((aligned(16))) uint32_t in[BL_ROWS * BL_IPD + 4];
    __shared__ __attribute__((aligned(16))) uint32_t hz2[(BL_ROWS / 2) * BL_TW];     // [row pair][x]: row 2m | row 2m+1 << 16
    const int tid = threadIdx.x;
    // persistent workgroup: a contiguous range of tiles in (level, frame, tile row, tile column) order -- each XCD's contiguous range of
    // logical ids stays inside few frames of one level; the next tile's loads are in flight while the current one is filtered
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    const long total = (long)P.bs_tiles[P.nlevels] * P.batch;
    const long t0 = total * lid / gridDim.x, t1 = total * (lid + 1) / gridDim.x;
    if (t0 >= t1) return;
    BlTile T;
    {
        T.level = 0;
        for (int l = 1; l < P.nlevels; l++) if (t0 >= (long)P.bs_tiles[l] * P.batch) T.level = l;
        bl_tile_level(P, T);
        const long rel = t0 - (long)P.bs_tiles[T.level] * P.batch;
        T.frame = (int)(rel / (T.ntx * T.nty));
        const int trem = (int)(rel - (long)T.frame * (T.ntx * T.nty));
        T.ty = trem / T.ntx; T.tx = trem - T.ty * T.ntx;
        bl_tile_frame(P, T);
    }
    const uint32_t klo = (uint32_t)P.gauss_q8[0] | ((uint32_t)P.gauss_q8[1] << 8) | ((uint32_t)P.gauss_q8[2] << 16) | ((uint32_t)P.gauss_q8[3] << 24);
    const uint32_t khi = (uint32_t)P.gauss_q8[4] | ((uint32_t)P.gauss_q8[5] << 8) | ((uint32_t)P.gauss_q8[6] << 16);
    const uint32_t k0 = P.gauss_q8[0], k1 = P.gauss_q8[1], k2 = P.gauss_q8[2], k3 = P.gauss_q8[3];
    const uint32_t wt[2][4] = {{k0 | (k1 << 16), k2 | (k3 << 16), k2 | (k1 << 16), k0},
                               {k0 << 16, k1 | (k2 << 16), k3 | (k2 << 16), k1 | (k0 << 16)}};
    // where this lane's staging share lands in LDS (same for every tile)
    const bool chunk = tid < 4 * BL_ROWS;
    const int sa = tid - 4 * BL_ROWS;
    const int sidx = chunk ? (tid >> 2) * BL_IPD + 4 + 4 * (tid & 3) : (sa >> 1) * BL_IPD + ((sa & 1) ? BL_IPD : 3);
    auto advance = [&](BlTile &X) {
        X.tx++;
        if (X.tx == X.ntx) { X.tx = 0; X.ty++; }
        if (X.ty == X.nty) {
            X.ty = 0; X.frame++;
            if (X.frame == P.batch) { X.frame = 0; X.level++; bl_tile_level(P, X); }
            bl_tile_frame(P, X);
        }
    };
    auto body = [&](uint4 &ld, BlTile &T, long t) {
        const int x0 = T.tx * BL_TW, y0 = T.ty * BL_TH, w = T.w, h = T.h, dpitch = T.dpitch;
        uint8_t *bdst = T.dst;
        if (chunk) *reinterpret_cast<uint4 *>(&in[sidx]) = ld;
        else if (sa < 2 * BL_ROWS) in[sidx] = ld.x;
        __syncthreads();
        if (t + 1 < t1) { advance(T); ld = bl_stage_load(T, tid); }                   // the next tile's loads are in flight during the passes
        // ---- row pass: two rows x four pixels per task, u16 sums (q8 kernel, sum 257 -> 255*257 fits)
        for (int i = tid; i < (BL_ROWS / 2) * (BL_TW / 4); i += 256) {
            const int rp = i >> 4, c4 = i & 15;
            const uint32_t *q = &in[2 * rp * BL_IPD + 3 + c4];
            uint32_t oa[4], ob[4];
            bl_row4(q[0], q[1], q[2], klo, khi, oa);
            bl_row4(q[BL_IPD], q[BL_IPD + 1], q[BL_IPD + 2], klo, khi, ob);
            uint4 pk;
            pk.x = oa[0] | (ob[0] << 16); pk.y = oa[1] | (ob[1] << 16); pk.z = oa[2] | (ob[2] << 16); pk.w = oa[3] | (ob[3] << 16);
            *reinterpret_cast<uint4 *>(&hz2[rp * BL_TW + 4 * c4]) = pk;
        }
        __syncthreads();
        // ---- column pass: rows come vertically paired, so a 7-tap column is four v_dot2_u32_u16
        {
            const int c4 = tid & 15, rg = tid >> 4;
            const int x = x0 + 4 * c4;
            if (x < w) {
                uint4 pr[4];
#pragma unroll
                for (int k = 0; k < 4; k++) pr[k] = *reinterpret_cast<const uint4 *>(&hz2[(rg + k) * BL_TW + 4 * c4]);
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int y = y0 + 2 * rg + rr;
                    if (y < h) {
                        uint32_t acc[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            uint32_t a = 32768u;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const uint32_t pv = j == 0 ? pr[k].x : j == 1 ? pr[k].y : j == 2 ? pr[k].z : pr[k].w;
                                a = bl_dot2(pv, wt[rr][k], a);
                            }
                            acc[j] = min(a, 0x00FFFFFFu);                  // byte 2 = min((sum + 2^15) >> 16, 255)
                        }
                        const uint32_t p01 = __builtin_amdgcn_perm(acc[1], acc[0], 0x0c0c0602u);
                        const uint32_t p23 = __builtin_amdgcn_perm(acc[3], acc[2], 0x0c0c0602u);
                        *reinterpret_cast<uint32_t *>(bdst + (uint32_t)__umul24((uint32_t)y, (uint32_t)dpitch) + x) = p01 | (p23 << 16);
                    }
                }
            }
        }
        // (the next tile's staging writes to `in` come after this tile's row pass: second barrier above;
        //  its row-pass writes to `hz2` come after its first barrier, i.e. after this column pass)
    };
    uint4 ld = bl_stage_load(T, tid);
    for (long t = t0; t < t1; t++) body(ld, T, t);
}

// Row-streaming form of the same filter (the default): no LDS, no barriers, so its waves fit into the wave slots k_fast_cells
// leaves free (that kernel is LDS-limited to ~17 waves per CU) and fill its idle issue cycles.  A lane owns 4 output columns and
// walks BLR_R output rows down: per source row one aligned dwordx3 (x-4 .. x+7), the row pass on v_dot4_u32_u8 as above, the
// horizontal sums of consecutive rows paired in a register ring of 6 (statically indexed: the row loop is unrolled by 6), the
// column pass = three v_dot2_u32_u16 on the pairs + one v_mad_u32_u24.  Chunks whose 12-byte window crosses the left / right
// image border (BORDER_REFLECT_101) are a separate lane class at the end of each (frame, level) lane range and assemble their
// windows bytewise.
template <bool EDGE>
__device__ __forceinline__ void blr_load(const uint8_t *src, int r, int spitch, int x, int w, uint32_t &d0, uint32_t &d1, uint32_t &d2)
{
    if (EDGE) {
        const uint8_t *row = src + (uint32_t)__umul24((uint32_t)r, (uint32_t)spitch);
        d0 = bl_load4(row, x - 4, w); d1 = bl_load4(row, x, w); d2 = bl_load4(row, x + 4, w);
    } else {
        const rs_u32x3 v = *reinterpret_cast<const rs_u32x3_a4 *>(src + ((uint32_t)__umul24((uint32_t)r, (uint32_t)spitch) + (uint32_t)(x - 4)));
        d0 = v.x; d1 = v.y; d2 = v.z;
    }
}
template <bool EDGE>
__device__ __forceinline__ void blr_band(const uint8_t *src, uint8_t *dst, int spitch, int dpitch, int w, int h, int x, int dy0,
                                         uint32_t klo, uint32_t khi, uint32_t k01, uint32_t k23, uint32_t k21, uint32_t k0)
{
    auto srow = [&](int i) { int r = dy0 - 3 + i; r = max(r, -r); return min(r, 2 * h - 2 - r); };    // BORDER_REFLECT_101 (h >= BLR_R + 4)
    // the six source rows of the NEXT group are in flight while this group is filtered (24 unique bytes per lane: the kernel is
    // bound by bytes in flight, not by issue); buffers and ring are statically indexed, the whole band is unrolled
    uint32_t ring[6][4], prev[4] = {0, 0, 0, 0};
    uint32_t buf[2][6][3];
#pragma unroll
    for (int u = 0; u < 6; u++) blr_load<EDGE>(src, srow(u), spitch, x, w, buf[0][u][0], buf[0][u][1], buf[0][u][2]);
    uint32_t doff = (uint32_t)__umul24((uint32_t)dy0, (uint32_t)dpitch) + (uint32_t)x;
#pragma unroll
    for (int g = 0; g < (BLR_R + 6) / 6; g++) {
        if (g + 1 < (BLR_R + 6) / 6) {
#pragma unroll
            for (int u = 0; u < 6; u++) blr_load<EDGE>(src, srow(6 * (g + 1) + u), spitch, x, w, buf[(g + 1) & 1][u][0], buf[(g + 1) & 1][u][1], buf[(g + 1) & 1][u][2]);
        }
#pragma unroll
        for (int u = 0; u < 6; u++) {
            const int i = 6 * g + u;
            uint32_t o[4];
            bl_row4(buf[g & 1][u][0], buf[g & 1][u][1], buf[g & 1][u][2], klo, khi, o);
            if (g > 0) {
                uint32_t acc[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t a = bl_dot2(ring[(u + 1) % 6][j], k01, 32768u);
                    a = bl_dot2(ring[(u + 3) % 6][j], k23, a);
                    a = bl_dot2(ring[(u + 5) % 6][j], k21, a);
                    a = __umul24(o[j], k0) + a;
                    acc[j] = min(a, 0x00FFFFFFu);                  // byte 2 = min((sum + 2^15) >> 16, 255)
                }
                const uint32_t p01 = __builtin_amdgcn_perm(acc[1], acc[0], 0x0c0c0602u);
                const uint32_t p23 = __builtin_amdgcn_perm(acc[3], acc[2], 0x0c0c0602u);
                if (dy0 + i - 6 < h) *reinterpret_cast<uint32_t *>(dst + doff) = p01 | (p23 << 16);
                doff += (uint32_t)dpitch;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) { ring[u][j] = prev[j] | (o[j] << 16); prev[j] = o[j]; }
        }
    }
}

__global__ __launch_bounds__(256) void k_blur_rows(OrbParams P, int frame0)
{
    const int per_frame = P.br_blocks[P.nlevels];
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    const int fr = (int)(lid / (unsigned)per_frame), rem = (int)(lid - (unsigned)fr * (unsigned)per_frame);     // uniform
    const int frame = frame0 + fr;
    int level = 0;
    for (int l = 1; l < P.nlevels; l++) if (rem >= P.br_blocks[l]) level = l;
    const OrbLevel &L = P.lv[level];
    const int w = L.w, h = L.h;
    const int nch = (w + 3) >> 2, nint = (w - 8) >> 2, nedge = nch - nint, nb = (h + BLR_R - 1) / BLR_R;
    const int idx = (rem - P.br_blocks[level]) * 256 + (int)threadIdx.x;
    if (idx >= nch * nb) return;
    const uint8_t *src = L.img + (size_t)frame * L.img_frame_stride;
    uint8_t *dst = L.blur + (size_t)frame * L.blur_frame_stride;
    const uint32_t klo = (uint32_t)P.gauss_q8[0] | ((uint32_t)P.gauss_q8[1] << 8) | ((uint32_t)P.gauss_q8[2] << 16) | ((uint32_t)P.gauss_q8[3] << 24);
    const uint32_t khi = (uint32_t)P.gauss_q8[4] | ((uint32_t)P.gauss_q8[5] << 8) | ((uint32_t)P.gauss_q8[6] << 16);
    const uint32_t k0 = P.gauss_q8[0], k1 = P.gauss_q8[1], k2 = P.gauss_q8[2], k3 = P.gauss_q8[3];
    const uint32_t k01 = k0 | (k1 << 16), k23 = k2 | (k3 << 16), k21 = k2 | (k1 << 16);
    if (idx < nint * nb) {
        const int band = idx / nint, c = 1 + idx - band * nint;
        blr_band<false>(src, dst, L.img_pitch, L.blur_pitch, w, h, 4 * c, band * BLR_R, klo, khi, k01, k23, k21, k0);
    } else {
        const int e = idx - nint * nb, band = e / nedge, ce = e - band * nedge;
        const int c = ce == 0 ? 0 : nint + ce;
        blr_band<true>(src, dst, L.img_pitch, L.blur_pitch, w, h, 4 * c, band * BLR_R, klo, khi, k01, k23, k21, k0);
    }
}

// ----------------------------------------------------------------------------------
// A7 on the matrix cores (round 3).  The blur is exact integer arithmetic (taps q8, no intermediate rounding, one (sum + 2^15) >> 16 at the
// end), so it can be regrouped freely: a 64 x 64 window of pixels times a banded 64 x 16 matrix of taps is the row pass for 16 output
// columns, and the column pass is the same product along the other axis.  Why: k_fast_cells and the blur share the CUs and are bound by the
// SUM of their vector instructions; k_blur_rows costs 14 per pixel, this form ~6, the multiply-adds go to the otherwise idle
// matrix pipe.  No LDS (k_fast_cells owns it), no cross-lane movement:
//   pass 1  C1[row][out col] = sum_k A[row][k] B[k][out col]: A = the window's pixels as int8 (p - 128: one xor per dword), lane (row & 15,
//           g = lane >> 4) holds the 16 bytes of chunk g of its row -- ONE 16-byte load; B = the taps as a band, from a host-built table per
//           (level, tile column, block) that also folds BORDER_REFLECT_101 in (a reflected column's tap is added to the column it mirrors)
//           and mirrors the chunk rule below; the accumulators start at 128 * (sum of taps), which undoes the bias: C1 = the plain 16-bit row sum.
//   pass 2  C2[out col][out row] = sum_k A2[out col][k] B2[k][out row]: A2 = C1 itself -- its layout (column on the lane, rows 4g + r in the
//           registers of the four row tiles) IS an A operand whose k slot (g, 4t + r) means window row 16t + 4g + r; the band table is built
//           in that slot order (any order works as long as both operands agree, tools/mfma_i8_probe.hip).  16-bit sums go in as two int8
//           products (high and low byte, each biased), 256 * hi + lo + 2^15 is formed in the epilogue; the result tile has 4 consecutive
//           COLUMNS of one output row per lane: one dword store.
// A wave owns a 32-column tile column and walks down in steps of 58 rows (64-row windows, 3 rows of apron each side; rows are reflected by
// index at load time).  Chunk rule (the table's too): chunk g of the window starts at 32 tx - 16 + 16 g, moved to 0 when negative and to
// w - 16 when it would cross the row's end -- loads never leave [0, w) of a row (level 0 may be the caller's buffer).
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4i bm_as_v4i(uint4 v) { v4i r; r[0] = (int)v.x; r[1] = (int)v.y; r[2] = (int)v.z; r[3] = (int)v.w; return r; }
// TILED: the one store goes to the tiled blurred level (orb_internal.h, ORB_BLUR_TILE_OFF) -- col is a multiple of 4 and X0 + 16 cb of 16, so the
// dword stays inside one tile row and the 16 rows x 16 bytes of a store instruction fill 2-3 whole 128-byte tiles of one tile column instead of
// sixteen partial lines.  Nothing else differs.
template <bool TILED>
__global__ __launch_bounds__(256) void k_blur_mfma(OrbParams P, int frame0, int nframes)
{
    const int per_frame = P.bm_cols[P.nlevels];
    // XCD-contiguous order: the four tile columns of a workgroup span 128 + 32 columns, so raw neighbours (dealt to different L2s) fetched
    // the 128-byte lines at their seams twice or three times (2.5 GB read per 1024 VGA frames against 0.98 GB of pixels, profiles/r04_pmc_traffic)
    const unsigned wid = xcd_logical_id(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int fr = (int)(wid / (unsigned)per_frame), rem = (int)(wid - (unsigned)fr * (unsigned)per_frame);
    if (fr >= nframes) return;
    int level = 0;
    for (int l = 1; l < P.nlevels; l++) if (rem >= P.bm_cols[l]) level = l;
    const OrbLevel &L = P.lv[level];
    const int w = L.w, h = L.h, spitch = L.img_pitch, dpitch = L.blur_pitch;
    const int tx = rem - P.bm_cols[level], X0 = 32 * tx, tiles_x = L.blur_tiles_x;
    const uint8_t *src = L.img + (size_t)(frame0 + fr) * L.img_frame_stride;
    uint8_t *dst = L.blur + (size_t)(frame0 + fr) * L.blur_frame_stride;
    int cx = X0 - 16 + 16 * g;
    cx = cx < 0 ? 0 : cx;
    if (cx + 16 > w) cx = w - 16;
    const uint4 *th = P.bm_th + ((size_t)(P.bm_cols[level] + tx) * 2) * 64 + lane;
    const v4i B0 = bm_as_v4i(th[0]), B1 = bm_as_v4i(th[64]);
    v4i TV[4];
#pragma unroll
    for (int b = 0; b < 4; b++) TV[b] = bm_as_v4i(P.bm_tv[b * 64 + lane]);
    const int init = P.bm_init;
    // the two start values stay in VGPRs for the whole walk and every MFMA reads them as its C operand: the empty asm makes them opaque, else
    // the register allocator re-creates them from scalar registers in front of each of the 16 pass-2 MFMAs (two v_mov_b64 apiece)
    v4i c_init = {init, init, init, init}, c_init_lo = {init + 32768, init + 32768, init + 32768, init + 32768};
    asm volatile("" : "+v"(c_init), "+v"(c_init_lo));
    const int nty = (h + 57) / 58;
    // the window of the NEXT step is in flight while this one is multiplied (one 16-byte load per lane and row tile)
    auto load_window = [&](int Y0, u32x4_unaligned (&raw)[4]) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int ya = Y0 - 3 + 16 * t + m;
            ya = ya < 0 ? -ya : ya;
            ya = ya >= h ? 2 * h - 2 - ya : ya;                       // BORDER_REFLECT_101; rows far below the image (last window) are never used
            ya = min(max(ya, 0), h - 1);
            raw[t] = *reinterpret_cast<const u32x4_unaligned *>(src + (uint32_t)(__umul24((uint32_t)ya, (uint32_t)spitch) + (uint32_t)cx));
        }
    };
    u32x4_unaligned raw[4];
    load_window(0, raw);
    for (int ty = 0; ty < nty; ty++) {
        const int Y0 = 58 * ty;
        v4i A[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            A[t][0] = (int)(raw[t].x ^ 0x80808080u); A[t][1] = (int)(raw[t].y ^ 0x80808080u); A[t][2] = (int)(raw[t].z ^ 0x80808080u); A[t][3] = (int)(raw[t].w ^ 0x80808080u);
        }
        if (ty + 1 < nty) load_window(Y0 + 58, raw);
        v4i C1[2][4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            C1[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], B0, c_init, 0, 0, 0);
            C1[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], B1, c_init, 0, 0, 0);
        }
#pragma unroll
        for (int cb = 0; cb < 2; cb++) {
            v4i Ahi, Alo;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint32_t pab = __builtin_amdgcn_perm((uint32_t)C1[cb][t][1], (uint32_t)C1[cb][t][0], 0x05040100u);      // (lo, hi) byte pairs of rows r = 0, 1
                const uint32_t pcd = __builtin_amdgcn_perm((uint32_t)C1[cb][t][3], (uint32_t)C1[cb][t][2], 0x05040100u);
                Alo[t] = (int)(__builtin_amdgcn_perm(pcd, pab, 0x06040200u) ^ 0x80808080u);
                Ahi[t] = (int)(__builtin_amdgcn_perm(pcd, pab, 0x07050301u) ^ 0x80808080u);
            }
            const int col = X0 + 16 * cb + 4 * g;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const v4i Chi = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ahi, TV[b], c_init, 0, 0, 0);
                const v4i Clo = __builtin_amdgcn_mfma_i32_16x16x64_i8(Alo, TV[b], c_init_lo, 0, 0, 0);
                uint32_t v[4];
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = min(((uint32_t)Chi[r] << 8) + (uint32_t)Clo[r], 0x00FFFFFFu);      // byte 2 = min((sum + 2^15) >> 16, 255)
                const uint32_t p01 = __builtin_amdgcn_perm(v[1], v[0], 0x0c0c0602u), p23 = __builtin_amdgcn_perm(v[3], v[2], 0x0c0c0602u);
                const int row = Y0 + 16 * b + m;
                if (TILED) {
                    if (16 * b + m < 58 && row < h && col < w) *reinterpret_cast<uint32_t *>(dst + ORB_BLUR_TILE_OFF(col, row, tiles_x)) = p01 | (p23 << 16);
                } else
                if (16 * b + m < 58 && row < h && col < w) *reinterpret_cast<uint32_t *>(dst + (uint32_t)(__umul24((uint32_t)row, (uint32_t)dpitch) + (uint32_t)col)) = p01 | (p23 << 16);
            }
        }
    }
}

// Host plan of the three kernels for the geometry in P.lv (no HIP call; P.rows_min_batch and P.gauss_q8 are set): the work prefixes
// bs_tiles / br_blocks / bm_cols ([nlevels] == 0: the geometry cannot take that kernel), bm_min_batch, bm_init, blur_tiled_ok and, where
// it returns true, k_blur_mfma's int8 operand tables (OrbParams::bm_th / bm_tv, 16 bytes per lane and block).
bool orb_plan_blur(OrbParams &P, std::vector<int8_t> &th, std::vector<int8_t> &tv)
{
    const int nlevels = P.nlevels;
    P.bs_tiles[0] = 0;
    for (int l = 0; l < nlevels; l++) P.bs_tiles[l + 1] = P.bs_tiles[l] + ((P.lv[l].w + BL_TW - 1) / BL_TW) * ((P.lv[l].h + BL_TH - 1) / BL_TH);
    {   // k_blur_rows: lanes = 4-column chunks x bands of BLR_R rows; needs BLR_R + 4 rows for its reflected row indices and one interior chunk
        bool ok = !getenv("ORBHIP_BLUR_TILES");
        P.br_blocks[0] = 0;
        for (int l = 0; l < nlevels; l++) {
            const int w = P.lv[l].w, h = P.lv[l].h;
            if (h < BLR_R + 4 || w < 16) ok = false;
            P.br_blocks[l + 1] = P.br_blocks[l] + (((w + 3) / 4) * ((h + BLR_R - 1) / BLR_R) + 255) / 256;
        }
        if (!ok) P.br_blocks[nlevels] = 0;
    }
    // k_blur_mfma operand tables: horizontal band per (level, 32-column tile column, 16-column block) with the image
    // borders folded in and the kernel's chunk rule mirrored; vertical band per 16-row output block in the slot order the accumulator
    // layout of pass 1 dictates.  Not used (k_blur_rows stays) for levels narrower than 32 or shorter than 8.
    // Round 4: the DEFAULT for images of up to 320 K pixels (VGA) in batches of 128 frames or more -- where the blur runs beside
    // k_fast_cells and the pair is bound by the sum of their vector instructions, the matrix-core form needs ~6 per pixel against 14
    // (measured after k_fast_cells lost 9 % of its own: 3.67 against 3.73 ms per 1024-frame VGA step, two A/B pairs; in round 3 the
    // two were even).  Alone it is the slower kernel (0.93 against 0.75 ms), and at 1080p / 4K, where the blur is a smaller share of
    // a step that is bound elsewhere, 12 % slower in the step: k_blur_rows stays for small batches and big images.
    // ORBHIP_BLUR_MFMA=1: every batch that takes the row-streaming kernels, any size; =0: never.  Bit-exact either way.
    const char *bm_env = getenv("ORBHIP_BLUR_MFMA");
    const bool bm_force = bm_env && atoi(bm_env) == 1, bm_off = bm_env && atoi(bm_env) == 0;
    // (crossover measured in one call per pair, frames/s matrix cores / rows: 640x480 x 1024: 278 k / 270 k, x 128: 184.3 k / 181.4 k;
    //  752x480 x 1024: 247.8 k / 249.7 k; 1280x720 x 512: 98.9 k / 104.0 k; 1920x1080 x 512: 44.2 k / 50.1 k)
    bool ok = !bm_off && (bm_force || (size_t)P.lv[0].w * P.lv[0].h <= (size_t)320 * 1024) && P.br_blocks[nlevels] > 0;      // level 0 = the image
    P.bm_min_batch = bm_force ? P.rows_min_batch : 128;
    int S = 0;
    for (int i = 0; i < 7; i++) { S += P.gauss_q8[i]; if (P.gauss_q8[i] < 0 || P.gauss_q8[i] > 63) ok = false; }     // two folded taps must fit int8
    if (255 * S > 65535) ok = false;                                                                              // row sums must fit 16 bits
    P.bm_cols[0] = 0;
    for (int l = 0; l < nlevels; l++) {
        if (P.lv[l].w < 32 || P.lv[l].h < 8) ok = false;
        P.bm_cols[l + 1] = P.bm_cols[l] + (P.lv[l].w + 31) / 32;
    }
    auto refl = [](int x, int n) { return x < 0 ? -x : (x >= n ? 2 * n - 2 - x : x); };
    th.assign((size_t)P.bm_cols[nlevels] * 2 * 64 * 16, 0); tv.assign((size_t)4 * 64 * 16, 0);
    for (int l = 0; l < nlevels && ok; l++) {
        const int w = P.lv[l].w;
        for (int tx = 0; tx < (w + 31) / 32; tx++) {
            int cxs[4];
            for (int g = 0; g < 4; g++) { int cx = 32 * tx - 16 + 16 * g; cx = cx < 0 ? 0 : cx; if (cx + 16 > w) cx = w - 16; cxs[g] = cx; }
            for (int cb = 0; cb < 2; cb++)
                for (int n = 0; n < 16; n++) {
                    const int xo = 32 * tx + 16 * cb + n;
                    if (xo >= w) continue;
                    for (int i = -3; i <= 3; i++) {
                        const int col = refl(xo + i, w);
                        int gp = -1;                                         // the first chunk that holds the column takes its tap
                        for (int g = 0; g < 4 && gp < 0; g++) if (col >= cxs[g] && col < cxs[g] + 16) gp = g;
                        if (gp < 0) { ok = false; break; }
                        int8_t &c = th[((((size_t)(P.bm_cols[l] + tx) * 2 + cb) * 64) + (size_t)(n + 16 * gp)) * 16 + (col - cxs[gp])];
                        c = (int8_t)(c + P.gauss_q8[i + 3]);
                    }
                }
        }
    }
    for (int b = 0; b < 4; b++)
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 16; j++) {
                const int n = lane & 15, g = lane >> 4, krow = 16 * (j >> 2) + 4 * g + (j & 3), d = krow - (16 * b + n);
                tv[((size_t)b * 64 + lane) * 16 + j] = (int8_t)((d >= 0 && d <= 6) ? P.gauss_q8[d] : 0);
            }
    P.bm_th = nullptr; P.bm_tv = nullptr; P.bm_init = 128 * S;
    // ORBHIP_BLUR_TILED=0: the matrix-core blur and k_orient_desc keep the row-major blurred pyramid (A/B runs, tests).  Same bytes out.
    P.blur_tiled_ok = !(getenv("ORBHIP_BLUR_TILED") && atoi(getenv("ORBHIP_BLUR_TILED")) == 0);
    if (!ok) P.bm_cols[nlevels] = 0;
    return ok;
}

// THE rule: which kernel blurs a batch of that many frames -- 0 = k_blur (LDS tiles), 1 = k_blur_rows, 2 = k_blur_mfma.  The matrix-core
// kernel also decides the layout of the blurred pyramid (tiled iff P.blur_tiled_ok), so the descriptor kernel must be chosen by this too.
int orb_blur_kernel(const OrbParams &P, int batch)
{
    if (P.bm_cols[P.nlevels] > 0 && batch >= P.bm_min_batch) return 2;
    if (P.br_blocks[P.nlevels] > 0 && batch >= P.rows_min_batch) return 1;
    return 0;
}

void orb_launch_blur(const OrbParams &P, hipStream_t s, int wgs_per_cu, int frame0, int nframes)
{
    const int kernel = orb_blur_kernel(P, P.batch);
    if (kernel == 2) {
        if (nframes < 0) nframes = P.batch - frame0;
        const long waves = (long)P.bm_cols[P.nlevels] * nframes;
        if (nframes > 0 && P.blur_tiled) hipLaunchKernelGGL(k_blur_mfma<true>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, P, frame0, nframes);
        else if (nframes > 0) hipLaunchKernelGGL(k_blur_mfma<false>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, P, frame0, nframes);
        return;
    }
    if (kernel == 1) {
        if (nframes < 0) nframes = P.batch - frame0;
        if (nframes > 0) hipLaunchKernelGGL(k_blur_rows, dim3((unsigned)P.br_blocks[P.nlevels] * (unsigned)nframes), dim3(256), 0, s, P, frame0);
        return;
    }
    if (frame0 > 0) return;                                    // the tile kernel always takes the whole batch (first call)
    const long total = (long)P.bs_tiles[P.nlevels] * P.batch;
    long nblocks = (long)(P.n_cus > 0 ? P.n_cus : 256) * wgs_per_cu;                           // persistent: 8 workgroups (32 waves) per CU when alone on the chip
    if (nblocks > total) nblocks = total;
    hipLaunchKernelGGL(k_blur, dim3((unsigned)nblocks), dim3(256), 0, s, P);
}

