// pyramid_kernels.hip -- the image pyramid of the ORB front-end (ORBextractor::ComputePyramid): k_resize (LDS tiles),
// k_resize_rows (row streaming), the host plan of the latter's tables and their launcher.
#include "orb_internal.h"
#include "wave_dpp.h"
#include <algorithm>
#include <cstdlib>

// ----------------------------------------------------------------------------------
// A2/A3  pyramid: level l from level l-1, cv::resize INTER_LINEAR 8UC1 fixed point
// (reference call ORBextractor.cc:1165; arithmetic SURVEY Appendix A.3).
// Each thread produces 4 horizontally adjacent output pixels and stores one dword.
// Coefficient tables are computed on the host in float exactly like OpenCV does.
// ----------------------------------------------------------------------------------
#define RS_TW 64              // output tile
#define RS_TH 32
#define RS_MAXC 144           // staged source columns (scale factor <= 2: 64*2 + apron, dword aligned)
#define RS_MAXR 68            // staged source rows
// Separable inside LDS: (A) stage the source footprint of a 64x32 output tile with aligned dword
// loads (vertical clamping of cv::resize baked into the staged rows), (B) horizontal pass for every
// staged row -> (S[sx]*a0 + S[sx+1]*a1) >> 4 as u16 (<= 32640), (C) vertical pass + rounding,
// 4 pixels per thread, one dword store.  Bit-identical to the scalar formula of Appendix A.3.
__global__ __launch_bounds__(256) void k_resize(OrbParams P, int level)
{
    __shared__ __attribute__((aligned(16))) uint32_t in[RS_MAXR * (RS_MAXC / 4)];
    __shared__ uint16_t hz[RS_MAXR * RS_TW];
    const OrbLevel &D = P.lv[level];
    const OrbLevel &S = P.lv[level - 1];
    const int tid = threadIdx.x;
    const int ntx = (D.w + RS_TW - 1) / RS_TW, nty = (D.h + RS_TH - 1) / RS_TH;
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    const int frame = lid / (ntx * nty), trem = lid - frame * (ntx * nty);
    const int dx0 = (trem % ntx) * RS_TW, dy0 = (trem / ntx) * RS_TH;
    const int dx_last = min(dx0 + RS_TW, D.w) - 1, dy_last = min(dy0 + RS_TH, D.h) - 1;
    const int ybase = D.yofs[dy0];                                   // may be -1
    const int nrows = min(D.yofs[dy_last] + 1 - ybase + 1, RS_MAXR);
    const int xbase = D.xofs[dx0] & ~15;
    const int nc16 = min((D.xofs[dx_last] + 1 - xbase) / 16 + 1, RS_MAXC / 16);
    const uint8_t *src = S.img + (size_t)frame * S.img_frame_stride;
    // coefficient tables of passes B and C: fetched now so that their latency hides behind the staging loads
    const int dxl = tid & 63, dxB = min(dx0 + dxl, D.w - 1);
    const int sxB = D.xofs[dxB], a0 = D.xalpha[2 * dxB], a1 = D.xalpha[2 * dxB + 1];
    int r0C[2], b0C[2], b1C[2];
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        const int dy = min(dy0 + 2 * (tid >> 4) + rr, D.h - 1);
        r0C[rr] = D.yofs[dy]; b0C[rr] = D.ybeta[2 * dy]; b1C[rr] = D.ybeta[2 * dy + 1];
    }
    // ---- A: 16-byte chunks, 8 chunk slots x 32 rows per sweep (index math is shifts only); the loads of a
    // sweep are issued before its LDS stores
    for (int c = tid & 7; c < nc16; c += 8) {
        const int x = xbase + 16 * c;
        for (int r0 = tid >> 3; r0 < nrows; r0 += 64) {
            uint4 reg[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int r = r0 + 32 * k;
                const int y = min(max(ybase + r, 0), S.h - 1);                   // clip(sy, 0, ssize.height)
                const uint8_t *row = src + (size_t)y * S.img_pitch;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (r < nrows) {
                    if (x + 15 < S.w) v = *reinterpret_cast<const uint4 *>(row + x);
                    else {
                        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll 1
                        for (int j = 0; j < 4; j++) {                             // right image edge only: keep it small
#pragma unroll
                            for (int m = 0; m < 4; m++) d[m] |= (uint32_t)row[min(x + 4 * m + j, S.w - 1)] << (8 * j);
                        }
                        v = make_uint4(d[0], d[1], d[2], d[3]);
                    }
                }
                reg[k] = v;
            }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int r = r0 + 32 * k;
                if (r < nrows) *reinterpret_cast<uint4 *>(&in[r * (RS_MAXC / 4) + 4 * c]) = reg[k];
            }
        }
    }
    __syncthreads();
    // ---- B
    {
        if (dx0 + dxl < D.w) {
            const int sx = sxB - xbase;
            const uint8_t *inb = reinterpret_cast<const uint8_t *>(in);
            for (int r = tid >> 6; r < nrows; r += 4) {
                const uint8_t *q = inb + r * RS_MAXC + sx;
                hz[r * RS_TW + dxl] = (uint16_t)((q[0] * a0 + q[1] * a1) >> 4);
            }
        }
    }
    __syncthreads();
    // ---- C
    {
        const int c4 = tid & 15, rg = tid >> 4;
        const int dx = dx0 + 4 * c4;
        if (dx < D.w) {
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                const int dy = dy0 + 2 * rg + rr;
                if (dy < D.h) {
                    const int r0 = r0C[rr] - ybase, b0 = b0C[rr], b1 = b1C[rr];
                    const uint2 t0 = *reinterpret_cast<const uint2 *>(&hz[r0 * RS_TW + 4 * c4]);
                    const uint2 t1 = *reinterpret_cast<const uint2 *>(&hz[(r0 + 1) * RS_TW + 4 * c4]);
                    const int u0[4] = {(int)(t0.x & 0xFFFF), (int)(t0.x >> 16), (int)(t0.y & 0xFFFF), (int)(t0.y >> 16)};
                    const int u1[4] = {(int)(t1.x & 0xFFFF), (int)(t1.x >> 16), (int)(t1.y & 0xFFFF), (int)(t1.y >> 16)};
                    uint32_t packed = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int v = (((b0 * u0[j]) >> 16) + ((b1 * u1[j]) >> 16) + 2) >> 2;
                        packed |= (uint32_t)(v & 255) << (8 * j);
                    }
                    *reinterpret_cast<uint32_t *>(D.img + (size_t)frame * D.img_frame_stride + (size_t)dy * D.img_pitch + dx) = packed;
                }
            }
        }
    }
}

// Row-streaming form (the default whenever 4 output columns read at most 8 consecutive source bytes, i.e. scale factors up to
// ~1.5): no barriers after the table copy.  A lane owns 4 output columns and a band of D.rs_rows output rows, and walks the band's
// SOURCE rows down in RS_STEPS steps.  Per step it loads its 8 bytes of one source row (L1/L2 hits after the first touch),
// v_perm_b32 drops (S[sx], S[sx+1]) into the halves of a dword and ONE v_dot2_u32_u16 per pixel is the horizontal pass
// S[sx]*a0 + S[sx+1]*a1; the four interpolated values of the previous step stay in registers, so a source row shared by two output
// rows (five of six at scale 1.2) is loaded and interpolated once.  The vertical pass runs every step -- v_mul_hi_u32_u24 on
// pre-shifted operands ((b << 12) * (h & ~15)) >> 32 == (b * (h >> 4)) >> 16, the two halves summed with the rounding constant by
// v_add3 and packed -- and only the store and its pointer advance are predicated by the step's emit flag: lanes of one wave may
// walk different bands, the walk itself never diverges.  The step table {source row, emit, b0 << 12, b1 << 12} is built by the
// host (orb_plan_resize below), RS_STEPS entries per band: a band is as tall as RS_STEPS steps allow on every band of the level
// (19 rows at 1.2, 16 at 1.44), steps a band does not need repeat its last row without emitting.
#define RS_STEPS ORB_RS_STEPS
static_assert(RS_STEPS % 8 == 0 && RS_STEPS >= 16, "k_resize_rows prefetches its steps in groups of eight, two groups at least");
typedef unsigned short rs_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t rs_hpass(uint2 q, uint32_t sel, uint32_t al)
{
    const uint32_t pq = __builtin_amdgcn_perm(q.y, q.x, sel);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(rs_u16x2, pq), __builtin_bit_cast(rs_u16x2, al), 0u, false) & ~15u;
}
__device__ __forceinline__ uint32_t rs_mulhi24(uint32_t a, uint32_t b)
{
    uint32_t d;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// Source bytes of one lane and one source row, as the 8 bytes starting at its (unaligned) base.  MODE 0: one unaligned
// global_load_dwordx2 (the texture addresser splits it: measured 30-40 % slower, as is a 4-byte-aligned dwordx2); MODE 1: aligned
// dwordx3 from base4 <= base, the bytes shifted back by two v_perm_b32 with a per-lane selector (shift 0..4: where the third dword
// would leave a row of the caller's level-0 buffer, base4 is one dword lower instead).
template <int MODE>
__device__ __forceinline__ uint2 rs_load8(const uint8_t *src, uint32_t off, uint32_t shsel)
{
    if (MODE == 0) return *reinterpret_cast<const uint2 *>(src + off);
    const rs_u32x3 v = *reinterpret_cast<const rs_u32x3_a4 *>(src + off);
    return make_uint2(__builtin_amdgcn_perm(v.y, v.x, shsel), __builtin_amdgcn_perm(v.z, v.y, shsel));
}
template <int MODE>
__global__ __launch_bounds__(256) void k_resize_rows(OrbParams P, int level, int nbx)
{
    extern __shared__ uint4 sl[];                       // (256 / nch + 2) * RS_STEPS entries: small, so that the kernel fits beside LDS-heavy ones
    const OrbLevel &D = P.lv[level];
    const OrbLevel &S = P.lv[level - 1];
    const unsigned lid = xcd_logical_id(blockIdx.x, gridDim.x);
    const unsigned frame = lid / (unsigned)nbx, bx = lid - frame * (unsigned)nbx;          // uniform
    const int rsr = D.rs_rows, nch = (D.w + 3) >> 2, nb = (D.h + rsr - 1) / rsr;
    // the step tables of this workgroup's bands -> LDS (the per-step lookups are then off the global-load chain)
    const int band_lo = (int)((bx * 256) / (unsigned)nch), band_hi = min((int)((bx * 256 + 255) / (unsigned)nch), nb - 1);
    for (int i = (int)threadIdx.x; i < (band_hi - band_lo + 1) * RS_STEPS; i += 256) sl[i] = reinterpret_cast<const uint4 *>(D.ytab)[band_lo * RS_STEPS + i];
    __syncthreads();
    const unsigned g = bx * 256 + threadIdx.x;
    if (g >= (unsigned)(nch * nb)) return;
    const unsigned band = g / (unsigned)nch, c = g - band * (unsigned)nch;
    const uint4 *xc = reinterpret_cast<const uint4 *>(D.xchunk) + 3 * c;
    const uint4 x0 = xc[0], x1 = xc[1];
    const uint4 x2 = xc[2];
    const uint32_t al3 = x2.x, shsel = x2.y;
    const uint32_t base = x0.x, sel0 = x0.y, sel1 = x0.z, sel2 = x0.w, sel3 = x1.x, al0 = x1.y, al1 = x1.z, al2 = x1.w;
    const uint8_t *src = S.img + (size_t)frame * S.img_frame_stride;
    uint8_t *dst = D.img + (size_t)frame * D.img_frame_stride;
    const uint4 *st = sl + ((int)band - band_lo) * RS_STEPS;
    const uint32_t spitch = (uint32_t)S.img_pitch;
    // the source rows of the NEXT eight steps are in flight while eight are computed (the kernel is bound by bytes in flight)
    uint2 q[2][8];
#pragma unroll
    for (int u = 0; u < 8; u++) q[0][u] = rs_load8<MODE>(src, __umul24(st[u].x, spitch) + base, shsel);
    uint32_t doff = __umul24(band * (uint32_t)rsr, (uint32_t)D.img_pitch) + 4 * c;
    uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;            // the previous step's row, interpolated
#pragma unroll
    for (int g = 0; g < RS_STEPS / 8; g++) {
        if (g + 1 < RS_STEPS / 8) {
#pragma unroll
            for (int u = 0; u < 8; u++) q[(g + 1) & 1][u] = rs_load8<MODE>(src, __umul24(st[8 * (g + 1) + u].x, spitch) + base, shsel);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint2 a = q[g & 1][u];
            const uint32_t n0 = rs_hpass(a, sel0, al0), n1 = rs_hpass(a, sel1, al1), n2 = rs_hpass(a, sel2, al2), n3 = rs_hpass(a, sel3, al3);
            if (8 * g + u > 0) {                                                               // a band's first step only fills h
                const uint4 t = st[8 * g + u];
                const uint32_t s0 = rs_mulhi24(t.z, h0) + rs_mulhi24(t.w, n0) + 2u;
                const uint32_t s1 = rs_mulhi24(t.z, h1) + rs_mulhi24(t.w, n1) + 2u;
                const uint32_t s2 = rs_mulhi24(t.z, h2) + rs_mulhi24(t.w, n2) + 2u;
                const uint32_t s3 = rs_mulhi24(t.z, h3) + rs_mulhi24(t.w, n3) + 2u;
                const uint32_t p01 = (s0 | (s1 << 16)) >> 2, p23 = (s2 | (s3 << 16)) >> 2;      // bytes 0 and 2 hold the pixels
                if (t.y) {
                    *reinterpret_cast<uint32_t *>(dst + doff) = __builtin_amdgcn_perm(p23, p01, 0x06040200u);
                    doff += (uint32_t)D.img_pitch;
                }
            }
            h0 = n0; h1 = n1; h2 = n2; h3 = n3;
        }
    }
}

// Host plan of k_resize_rows for one level > 0, from the level's cv::resize tables (xo / xa: source column and coefficient pair per
// output column, yo / yb: the same per output row).  xc: per 4 output columns the 8 source bytes they read (base clamped into the
// row), v_perm selectors that put (S[sx], S[sx+1]) into the two halves of a dword, and the coefficient pairs; yt: per band of output
// rows the walk down its source rows, one step per row: {clamped source row, emit, vertical coefficients pre-shifted for
// v_mul_hi_u32_u24} (layouts: OrbLevel::xchunk / ytab, orb_internal.h).  Sets the level's rs_rows and, where the level takes the
// kernel, its resize_mode.  False: the level keeps k_resize (its geometry does not fit, or ORBHIP_RESIZE_TILES is set).
bool orb_plan_resize(OrbParams &P, int level, const std::vector<int16_t> &xo, const std::vector<int16_t> &xa, const std::vector<int16_t> &yo,
                     const std::vector<int16_t> &yb, std::vector<uint32_t> &xc, std::vector<uint32_t> &yt)
{
    OrbLevel &L = P.lv[level];
    const int l = level, sw = P.lv[l - 1].w, sh = P.lv[l - 1].h, nch = (L.w + 3) / 4;
    xc.assign((size_t)nch * 12, 0); yt.clear();
    bool fits = sw >= 8 && nch >= 4;                            // nch: the kernel's LDS table holds 256 / nch + 2 bands
    const char *rm = getenv("ORBHIP_RESIZE_MODE");
    int mode = l > 1 || (sw % 4 == 0 && sw >= 12) ? 1 : 0;       // level 0 may alias the caller's images: never read past a row there
    if (rm && atoi(rm) == 0) mode = 0;
    for (int c = 0; c < nch && fits; c++) {
        const int base = std::min((int)xo[4 * c], sw - 8);
        // the aligned variant loads 12 bytes from base4 = base & ~3 and shifts them back with v_perm; level 0 may be the
        // caller's buffer, so there base4 is lowered where the third dword would leave the row (shift 4, width % 4 == 0)
        const int base4 = l > 1 ? (base & ~3) : std::min(base & ~3, sw - 12);
        xc[12 * c] = mode ? (uint32_t)base4 : (uint32_t)base;
        xc[12 * c + 9] = 0x03020100u + 0x01010101u * (uint32_t)(base - base4);
        for (int j = 0; j < 4; j++) {
            const int col = std::min(4 * c + j, L.w - 1);
            const int i0 = xo[col] - base, a0 = xa[2 * col], a1 = xa[2 * col + 1];
            int i1 = i0 + 1;
            if (i0 < 0 || i0 > 7 || a0 < 0 || a1 < 0) { fits = false; break; }
            if (i1 > 7) { if (a1 != 0) { fits = false; break; } i1 = i0; }
            xc[12 * c + 1 + j] = (uint32_t)i0 | 0x0c00u | ((uint32_t)i1 << 16) | 0x0c000000u;
            xc[12 * c + 5 + j] = (uint32_t)a0 | ((uint32_t)a1 << 16);
        }
    }
    for (int dy = 0; dy < L.h; dy++)
        if (yb[2 * dy] < 0 || yb[2 * dy + 1] < 0 || yb[2 * dy] > 2048 || yb[2 * dy + 1] > 2048) fits = false;
    // The steps of output rows [y0, y1): an output row (r0, r1) is emitted by the step that interpolates r1, with r0 the row of
    // the step before.  Where r0 is not that row (a band's first row; the first source row advanced by 2; r0 == r1 clamped at
    // the bottom after another row) a step without emit loads it first.  Returns the number of steps.
    auto band_steps = [&](int y0, int y1, std::vector<uint32_t> *out) {
        int n = 0, prev = -1;
        for (int dy = y0; dy < y1; dy++) {
            const int r0 = std::min(std::max((int)yo[dy], 0), sh - 1), r1 = std::min(std::max((int)yo[dy] + 1, 0), sh - 1);
            if (n == 0 || prev != r0) {
                if (out) { const uint32_t e[4] = {(uint32_t)r0, 0u, 0u, 0u}; out->insert(out->end(), e, e + 4); }
                n++;
            }
            if (out) { const uint32_t e[4] = {(uint32_t)r1, 1u, (uint32_t)yb[2 * dy] << 12, (uint32_t)yb[2 * dy + 1] << 12}; out->insert(out->end(), e, e + 4); }
            n++; prev = r1;
        }
        return n;
    };
    int rsr = ORB_RS_STEPS - 1;                                 // the tallest band whose walk fits ORB_RS_STEPS steps everywhere (1 row: 2 steps)
    for (; rsr > 1; rsr--) {
        bool ok = true;
        for (int y0 = 0; y0 < L.h && ok; y0 += rsr) ok = band_steps(y0, std::min(y0 + rsr, L.h), nullptr) <= ORB_RS_STEPS;
        if (ok) break;
    }
    L.rs_rows = rsr;
    for (int y0 = 0; y0 < L.h && fits; y0 += rsr) {
        const size_t at = yt.size();
        band_steps(y0, std::min(y0 + rsr, L.h), &yt);
        while (yt.size() < at + 4 * ORB_RS_STEPS) {             // steps the band does not need: its last row again, no emit
            const uint32_t e[4] = {yt[yt.size() - 4], 0u, 0u, 0u};
            yt.insert(yt.end(), e, e + 4);
        }
    }
    if (!fits || getenv("ORBHIP_RESIZE_TILES")) return false;
    L.resize_mode = mode;
    return true;
}

void orb_launch_resize(const OrbParams &P, int level, hipStream_t s)
{
    const OrbLevel &D = P.lv[level];
    if (D.xchunk && P.batch >= P.rows_min_batch) {
        const int nch = (D.w + 3) >> 2, nb = (D.h + D.rs_rows - 1) / D.rs_rows, nbx = (nch * nb + 255) / 256;
        const dim3 grid((unsigned)nbx * (unsigned)P.batch);
        const size_t lds = (size_t)((256 / nch + 2) * RS_STEPS) * sizeof(uint4);          // <= 25 KB (nch >= 4)
        if (D.resize_mode == 1) hipLaunchKernelGGL(k_resize_rows<1>, grid, dim3(256), lds, s, P, level, nbx);
        else hipLaunchKernelGGL(k_resize_rows<0>, grid, dim3(256), lds, s, P, level, nbx);
        return;
    }
    const unsigned nblocks = (unsigned)(((D.w + RS_TW - 1) / RS_TW) * ((D.h + RS_TH - 1) / RS_TH)) * (unsigned)P.batch;
    hipLaunchKernelGGL(k_resize, dim3(nblocks), dim3(256), 0, s, P, level);
}

