// desc_kernels.hip -- orientation and descriptors of the ORB front-end: k_orient_desc (row-major blurred pyramid),
// k_orient_desc_tiled (tiled blurred pyramid, after k_blur_mfma) and their launcher.
#include "orb_internal.h"
#include "wave_dpp.h"

// ----------------------------------------------------------------------------------
// A6 + A8  IC_Angle (ORBextractor.cc:75-102) + steered BRIEF (ORBextractor.cc:106-145),
// one wave per keypoint.  Orientation: 2 patch rows per step (lanes 0-30 / 32-62),
// int32 moments, wave reduction.  Descriptor: lane l evaluates tests l, l+64, l+128,
// l+192; a 64-bit ballot is 8 descriptor bytes (LSB-first, as the reference packs them).
// ----------------------------------------------------------------------------------
__constant__ int8_t c_pattern[1024] = {
#include "orb_pattern.inc"
};

// cv::fastAtan2 scalar path, op-by-op, no contraction.
__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
    const float scale = (float)(180.0 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale;
    const float p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, (float)2.2204460492503131e-16));
        c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, (float)2.2204460492503131e-16));
        c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// "orb_sincos" (DESIGN.md): fixed IEEE-double fma sequence, identical to the oracle's.
__device__ __forceinline__ void sincos_det(double x, double *s_out, double *c_out)
{
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const int k = (int)__dadd_rn(__dmul_rn(x, TWO_OVER_PI), 0.5);
    const double dk = (double)k;
    double r = fma(-dk, PIO2_HI, x);
    r = fma(-dk, PIO2_LO, r);
    const double z = __dmul_rn(r, r);
    double ps = fma(z, S6, S5); ps = fma(z, ps, S4); ps = fma(z, ps, S3); ps = fma(z, ps, S2); ps = fma(z, ps, S1);
    const double s = fma(__dmul_rn(r, z), ps, r);
    double pc = fma(z, C6, C5); pc = fma(z, pc, C4); pc = fma(z, pc, C3); pc = fma(z, pc, C2); pc = fma(z, pc, C1);
    const double c = fma(__dmul_rn(z, z), pc, fma(z, -0.5, 1.0));
    switch (k & 3) {
    case 0: *s_out = s; *c_out = c; break;
    case 1: *s_out = c; *c_out = -s; break;
    case 2: *s_out = -s; *c_out = -c; break;
    default: *s_out = -c; *c_out = s; break;
    }
}

// Sixteen lanes per keypoint (four keypoints per wave), persistent waves with a grid stride; a trip's head (frame, level, count, key,
// position) is fetched during the wave's previous trip (od_head_issue below).
// Per keypoint the 16 lanes stage the 31x31 un-blurred patch and the 39x39 blurred patch into LDS
// with coalesced dword loads, accumulate the 749-pixel moments from LDS (two patch columns per
// lane, reduced over the 16 lanes), evaluate cv::fastAtan2 / orb_sincos once per keypoint (the four
// keypoints of a wave share those instructions), and each lane produces 16 of the 256 rBRIEF bits
// = two consecutive descriptor bytes.
#define OD_UP 48              // un-blurred patch pitch: 31 + up to 3 alignment bytes, staged as three 16-byte chunks
#define OD_BP 48              // blurred patch pitch: 39 + up to 3, three 16-byte chunks
#define OD_KP_LDS ((39 * OD_BP) / 4)                     // dwords per keypoint: the un-blurred patch (moments) and then the blurred one (rBRIEF) share it
#define OD_THREADS 128        // 8 keypoints per workgroup: 19.6 KB of LDS -> 8 workgroups (16 waves) per CU
// 16-byte fetch at a dword-aligned x: one dwordx4 per lane instead of four dword loads (the kernel's time
// follows the number of load wave-instructions).  A chunk may run up to 16 bytes past the end of its row:
// those bytes are never sampled (patches lie inside the image) and the read stays inside the buffer -- the
// un-blurred patch ends at image row <= h-5 (so the overrun lands in a later row, also when level 0 aliases
// the caller's frames), the blurred levels are allocated with 64 bytes of slack (orbhip_extractor_reserve).
__device__ __forceinline__ uint4 od_load16(const uint8_t *img, uint32_t row_off, int x)
{
    return *reinterpret_cast<const uint4 *>(img + (row_off + (uint32_t)x));      // uniform base + 32-bit lane offset
}

#ifdef OD_PROF
// debug build only (make EXTRA=-DOD_PROF): wave-cycles of k_orient_desc / k_orient_desc_tiled by phase, summed over all waves -- [0] top of trip ->
// header known, [1] -> patch loads issued, [2] -> patch data arrived, [3] -> moments done (with the LDS writes of the un-blurred patch), [4] ->
// angle / sine / cosine done (with the LDS writes of the blurred patch), [5] -> BRIEF done and stored, [6] trips of groups beyond their level's
// count; [7] trips with keypoints, [8] skipped trips, [9] whole kernel, [10] prologue (tables).  The waits for memory sit on their own
// boundaries (vmcnt(0)), so the build is slower than the product and the shares are those of the instrumented kernel.
__device__ unsigned long long g_od_prof[12];
extern "C" int orbhip_debug_od_prof(unsigned long long *out12, int reset)
{
    if (out12 && hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_od_prof), 96) != hipSuccess) return -1;
    if (reset) { unsigned long long z[12] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_od_prof), z, 96) != hipSuccess) return -1; }
    return 0;
}
#define OD_PROF_BEGIN() unsigned long long od_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, od_prev = __builtin_readcyclecounter(); const unsigned long long od_t0 = od_prev
#define OD_T(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); od_acc[i] += t_ - od_prev; od_prev = t_; } while (0)
#define OD_N(i) do { od_acc[i] += 1; } while (0)
#define OD_VMWAIT() __builtin_amdgcn_s_waitcnt(0x0F70)              // vmcnt(0)
#define OD_PROF_END() do { od_acc[9] = __builtin_readcyclecounter() - od_t0; \
                           if ((threadIdx.x & 63) == 0) for (int i = 0; i < 11; i++) atomicAdd(&g_od_prof[i], od_acc[i]); } while (0)
#else
#define OD_PROF_BEGIN() do { } while (0)
#define OD_T(i) do { } while (0)
#define OD_N(i) do { } while (0)
#define OD_VMWAIT() do { } while (0)
#define OD_PROF_END() do { } while (0)
#endif

// ---- the head of a trip (both readers): everything a wave must know before it can fetch the patches of its group of 4 work slots.
// Nothing of it depends on what a trip computes, so the head of the wave's NEXT trip is fetched while the current one waits for its patches
// (od_head_issue right after the patch loads) and is consumed at the top of the next trip: from its second trip on a wave meets no memory
// round trip before its patch loads.  Within the head nothing waits for anything either: the level comes from the kp_base values held in
// scalar registers, and count, key and position are three independent loads at the work slot -- the octree stores the keys in work order
// (lvl_wkey) beside the positions (lvl_perm); an entry beyond the level's count is stale, it is loaded and never used (`valid` comes after).
struct OdHead {
    int frame, slot0, kp_base;            // wave-uniform: frame, first of the 4 work slots, start of their level's slice
    const uint8_t *uimg, *bimg;           // the frame's un-blurred / blurred level
    int upitch, bgeom;                    // un-blurred pitch; blurred pitch (row-major) or tiles per tile row (tiled)
    int nk;                               // the level's count (one value per wave, fetched by a vector load so that it can stay in flight)
    uint32_t key;                         // the work slot's keypoint
    int pos;                              // its position inside the level's slice: results stay in the reference's slots
};
// kp_base of every level in scalar registers, INT_MAX beyond nlevels: the level of a slot is a count of compares, no memory in the loop
__device__ __forceinline__ void od_level_bases(const OrbParams &P, int (&kb)[ORB_MAX_LEVELS])
{
#pragma unroll
    for (int l = 0; l < ORB_MAX_LEVELS; l++) kb[l] = __builtin_amdgcn_readfirstlane(l < P.nlevels ? P.lv[l].kp_base : 0x7FFFFFFF);
}
template <bool TILED>
__device__ __forceinline__ void od_head_issue(const OrbParams &P, const int (&kb)[ORB_MAX_LEVELS], int frame, int slot0, int sub, OdHead &h)
{
    // every per-level staging slice is a multiple of 4 slots (orbhip_extractor_reserve), so the 4 keypoints of a wave share frame and
    // level: level parameters stay in scalar registers
    int lvl = 0;
#pragma unroll
    for (int l = 1; l < ORB_MAX_LEVELS; l++) lvl += slot0 >= kb[l] ? 1 : 0;
    lvl = __builtin_amdgcn_readfirstlane(lvl);
    const OrbLevel &L = P.lv[lvl];
    h.frame = frame; h.slot0 = slot0; h.kp_base = L.kp_base;
    h.uimg = L.img + (size_t)frame * L.img_frame_stride; h.bimg = L.blur + (size_t)frame * L.blur_frame_stride;
    h.upitch = L.img_pitch & 0xFFFF; h.bgeom = (TILED ? L.blur_tiles_x : L.blur_pitch) & 0xFFFF;      // known-small operands: 24-bit multiplies
    const size_t at = (size_t)frame * P.kps_per_frame + (size_t)(slot0 + sub);        // the work slot: inside the allocation whatever the count
    h.nk = P.lvl_count[frame * P.nlevels + lvl];
    if (P.batch >= ORB_PERM_MIN_BATCH) { h.key = P.lvl_wkey[at]; h.pos = (int)P.lvl_perm[at]; }
    else { h.key = P.lvl_kp[at]; h.pos = slot0 + sub - h.kp_base; }                   // few frames: the slot order (oct_output)
}
// the wave's next group: (fk, g) = frame number on this XCD and group inside the frame, carried from trip to trip (no division)
#define OD_NEXT_GROUP() do { g += step_g; fk += step_f; if (g >= gpf) { g -= gpf; fk++; } } while (0)

// ---- what the two kernels below share word for word.  MACROS expanded in place, on purpose: the same text as force-inlined functions is
// simplified on its own before it is inlined and disturbs the register allocation of both kernels (profiles/refactor_orb_streams.txt).
// They use the kernels' names: tid, l16, P, pat_t, od_msk, lds_all; later ones use what earlier ones declare.
// LDS tables: pat_t[t][l] = test 16 l + t as floats x0, y0, x1, y1; od_msk[|v|][j] = bytes of columns -15+4j .. -12+4j inside the circular patch
#define OD_TABLES() \
    for (int e = tid; e < 256; e += OD_THREADS) { \
        const int l = e & 15, t = e >> 4;         /* 16 x 16 entries */ \
        const int8_t *pp = &c_pattern[4 * (16 * l + t)]; \
        pat_t[t * 16 + l] = make_float4((float)pp[0], (float)pp[1], (float)pp[2], (float)pp[3]); \
    } \
    if (tid < 16 * 8) { \
        const int d = P.umax[tid >> 3], j = tid & 7; \
        uint32_t m = 0; \
        for (int k = 0; k < 4; k++) { const int u = -ORB_HALF_PATCH + 4 * j + k; if (u >= -d && u <= d) m |= 0xFFu << (8 * k); } \
        od_msk[tid] = m; \
    }
// XCD-aware work split (speed only): workgroups with equal blockIdx.x % 8 share an XCD and its L2, so
// frame f is handled by the workgroups of XCD (f % 8): every 128-byte line of a frame's pyramid is then
// fetched from HBM by one L2 instead of eight.  Declares the wave's LDS region (up32 / bp32 / bp), its trip state (fk, g: OD_NEXT_GROUP)
// and the level bases kb.
#define OD_WORK_SPLIT() \
    const int xcd = blockIdx.x & 7, nblk_x = gridDim.x >> 3;             /* gridDim.x is a multiple of 8 */ \
    const int wave_x = __builtin_amdgcn_readfirstlane((int)(blockIdx.x >> 3) * (OD_THREADS / 64) + (tid >> 6)), nwaves_x = nblk_x * (OD_THREADS / 64); \
    const int gpf = (P.kps_per_frame + 3) >> 2;                          /* groups of 4 slots per frame */ \
    const int nframes_x = (P.batch - xcd + 7) >> 3;                      /* frames xcd, xcd+8, ... */ \
    uint32_t *up32 = lds_all[(tid >> 4)], *bp32 = up32; \
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(bp32); \
    const float factor_pi = (float)(3.1415926535897932384626433832795 / 180.f); \
    /* the wave's trips: groups wave_x, wave_x + nwaves_x, ... of the XCD's nframes_x * gpf, as (frame number fk, group g) stepped without a division */ \
    const int step_f = __builtin_amdgcn_readfirstlane(nwaves_x / gpf), step_g = __builtin_amdgcn_readfirstlane(nwaves_x - step_f * gpf); \
    int fk = __builtin_amdgcn_readfirstlane(wave_x / gpf), g = __builtin_amdgcn_readfirstlane(wave_x - fk * gpf); \
    int kb[ORB_MAX_LEVELS]; \
    od_level_bases(P, kb)
// Top of a trip (inside the trip loop: it may `continue`): takes the head fetched during the previous trip as h and steps to the next group;
// a group beyond its level's count only sends the next head out.  Declares frame, valid (this lane's work slot holds a keypoint), slot
// (where its results go, used under `valid` only) and the keypoint's x, y (ORBextractor.cc:868-869)
#define OD_TRIP_HEAD(TILED) \
    const OdHead h = nx; \
    OD_NEXT_GROUP(); \
    OD_VMWAIT(); \
    const int nk = __builtin_amdgcn_readfirstlane(h.nk); \
    if (h.slot0 - h.kp_base >= nk) { \
        if (fk < nframes_x) od_head_issue<TILED>(P, kb, xcd + 8 * fk, 4 * g, sub, nx); \
        OD_T(6); OD_N(8); \
        continue; \
    } \
    const int frame = h.frame; \
    const bool valid = (h.slot0 + sub - h.kp_base) < nk;             /* work slot: the (slot0 + sub)-th keypoint of the level in spatial order */ \
    const int slot = h.kp_base + h.pos; \
    int x = 19, y = 19; \
    if (valid) { x = ORB_KEY_X(h.key) + ORB_MINB; y = ORB_KEY_Y(h.key) + ORB_MINB; } \
    OD_T(0); OD_N(7)
// IC_Angle (ORBextractor.cc:75-102) on the un-blurred patch at up32 (pitch OD_UP, first column at byte uoff): declares m10, m01, this lane's share.
// Lane (j = l16 & 7, parity = l16 >> 3) sweeps patch columns -15+4j .. -12+4j of every second row:
// m10 = sum (u+16) I - 16 sum I and m01 = sum v * rowsum, both on v_dot4_u32_u8 (exact integers)
#define OD_MOMENTS() \
    int m10, m01 = 0; \
    { \
        const int j = l16 & 7, par = l16 >> 3; \
        const uint32_t wts = 0x04030201u + 0x04040404u * (uint32_t)j; \
        uint32_t accP = 0, accS = 0; \
        _Pragma("unroll 4") \
        for (int i = 0; i < 16; i++) { \
            const int v = -ORB_HALF_PATCH + 2 * i + par, vc = min(v, ORB_HALF_PATCH); \
            const uint32_t *rq = up32 + (vc + ORB_HALF_PATCH) * (OD_UP / 4) + j; \
            uint32_t wv = __builtin_amdgcn_alignbyte(rq[1], rq[0], (uint32_t)uoff) & od_msk[(vc < 0 ? -vc : vc) * 8 + j]; \
            if (v > ORB_HALF_PATCH) wv = 0; \
            const uint32_t sr = __builtin_amdgcn_udot4(wv, 0x01010101u, 0u, false); \
            accP = __builtin_amdgcn_udot4(wv, wts, accP, false); \
            accS += sr; \
            m01 += v * (int)sr; \
        } \
        m10 = (int)accP - 16 * (int)accS; \
    }
// Steered BRIEF: this lane's 16 tests on the blurred patch bytes at bp -> `bits` (declared here; shifted in MSB-first, so t runs down).
// cvRound by the 1.5*2^23 trick: fl(r + M) holds round-half-even(r) in its low mantissa bits, i.e. as_int = K + n with K = 0x4B400000;
// row * pitch + col is then shifts and adds on the raw bits, ROW(r) = r * pitch, with the (pitch + 1) * K excess folded into offk, the
// patch-centre offset (the caller's)
#define OD_ROW48(r) (((r) << 5) + ((r) << 4))
#define OD_ROW64(r) ((r) << 6)
#define OD_BRIEF(ROW) \
    const float MAGIC = 12582912.0f; \
    uint32_t bits = 0; \
    _Pragma("unroll 4") \
    for (int t = 15; t >= 0; t--) { \
        const float4 pk = pat_t[t * 16 + l16]; \
        const uint32_t r0 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(pk.x, b), __fmul_rn(pk.y, a)), MAGIC)); \
        const uint32_t c0 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(pk.x, a), __fmul_rn(pk.y, b)), MAGIC)); \
        const uint32_t r1 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(pk.z, b), __fmul_rn(pk.w, a)), MAGIC)); \
        const uint32_t c1 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(pk.z, a), __fmul_rn(pk.w, b)), MAGIC)); \
        const uint32_t i0 = ROW(r0) + c0 + offk, i1 = ROW(r1) + c1 + offk; \
        const uint32_t t0 = bp[i0], t1 = bp[i1]; \
        bits = __builtin_amdgcn_alignbit(bits, t0 - t1, 31);        /* bits << 1 | (t0 < t1) */ \
    }
// results stay in the reference's slots
#define OD_STORE() \
    if (valid) { \
        uint8_t *desc = P.lvl_desc + ((size_t)frame * P.kps_per_frame + slot) * 32; \
        reinterpret_cast<uint16_t *>(desc)[l16] = (uint16_t)bits;              /* tests 16*l16 .. 16*l16+15 = bytes 2*l16, 2*l16+1 */ \
        if (l16 == 0) P.lvl_angle[(size_t)frame * P.kps_per_frame + slot] = angle; \
    }

// (four waves per SIMD = the 16 waves per CU its LDS allows: 128 VGPRs, no spill; left to itself the compiler takes 138 for the carried head)
__global__ __launch_bounds__(OD_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_orient_desc(OrbParams P)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OD_THREADS / 16][OD_KP_LDS];
    __shared__ float4 pat_t[16 * 16];            // pat_t[t][l] = test 16*l + t as floats x0,y0,x1,y1
    __shared__ uint32_t od_msk[16 * 8];          // od_msk[|v|][j]: bytes of columns -15+4j..-12+4j inside the circular patch
    const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, sub = lane >> 4;
    OD_PROF_BEGIN();
    OD_TABLES();
    __syncthreads();
    OD_WORK_SPLIT();
    OdHead nx = {};
    if (fk < nframes_x) od_head_issue<false>(P, kb, xcd + 8 * fk, 4 * g, sub, nx);          // the first trip's head: the only one a wave waits for
    OD_T(10);
    while (fk < nframes_x) {
        OD_TRIP_HEAD(false);
        // ---- stage both patches (16 lanes per keypoint)
        const int uxs = (x - 15) & ~3, uoff = (x - 15) - uxs;        // un-blurred: cols x-15..x+15
        const int bxs = (x - 19) & ~3, boff = (x - 19) - bxs;        // blurred:    cols x-19..x+19
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // previous keypoints' LDS reads are done
        // the 16 lanes sweep the patch rows in 16-byte chunks (3 per row): 6 + 8 dwordx4 loads per lane, all issued
        // before the first LDS store so that they are in flight together; the blurred chunks wait in registers
        // until the moments are done with the shared LDS region
        uint4 br[8];
#pragma unroll
        for (int k = 0; k < 8; k++) br[k] = make_uint4(0, 0, 0, 0);
        uint4 ur[6];
        if (valid) {
            const uint8_t *uimg = h.uimg, *bimg = h.bimg;
            const int upitch = h.upitch, bpitch = h.bgeom;
            const uint32_t urow = (uint32_t)(((y - 15) & 0xFFFF) * upitch), brow = (uint32_t)(((y - 19) & 0xFFFF) * bpitch);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;      // i / 3 for i < 128
                ur[k] = i < 31 * 3 ? od_load16(uimg, urow + (uint32_t)(r * upitch), uxs + 16 * c3) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;      // i / 3 for i < 128
                if (i < 39 * 3) br[k] = od_load16(bimg, brow + (uint32_t)(r * bpitch), bxs + 16 * c3);
            }
        }
        if (fk < nframes_x) od_head_issue<false>(P, kb, xcd + 8 * fk, 4 * g, sub, nx);     // the next trip's head travels with this trip's patches
        OD_T(1); OD_VMWAIT(); OD_T(2);
        if (valid) {
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;      // i / 3 for i < 128
                if (i < 31 * 3) *reinterpret_cast<uint4 *>(&up32[r * (OD_UP / 4) + 4 * c3]) = ur[k];
            }
        }
        wave_lds_sync();
        // ---- IC_Angle (ORBextractor.cc:75-102)
        OD_MOMENTS();
        OD_T(3);
        // the moments' LDS reads are done: the blurred patch takes the region over
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;      // i / 3 for i < 128
                if (i < 39 * 3) *reinterpret_cast<uint4 *>(&bp32[r * (OD_BP / 4) + 4 * c3]) = br[k];
            }
        }
        m10 = row16_allreduce_add_dpp(m10); m01 = row16_allreduce_add_dpp(m01);        // the keypoint's 16 lanes = one DPP row
        const float angle = fast_atan2_deg((float)m01, (float)m10);
        // ---- steered BRIEF on the blurred level (ORBextractor.cc:106-145)
        double sd, cd;
        sincos_det((double)__fmul_rn(angle, factor_pi), &sd, &cd);
        const float a = (float)cd, b = (float)sd;
        OD_T(4);
        wave_lds_sync();
        const uint32_t offk = (uint32_t)(19 * OD_BP + boff + 19) - 49u * 0x4B400000u;      // row * 48 + col: the patch centre less the 49 K excess
        OD_BRIEF(OD_ROW48);
        OD_STORE();
        OD_T(5);
    }
    OD_PROF_END();
}

// The tiled form (OrbParams::blur_tiled: the matrix-core blur wrote the blurred levels in 16 x 8-pixel tiles, one 128-byte line each).
// Same arithmetic, same bytes out; only the staging differs.  The rBRIEF samples of a keypoint lie in a disc of radius 18.4 (the largest
// pattern norm) around it: rows y-18 .. y+18, per row the columns [-blur_hw, blur_hw].  A patch row's 37 columns span 3 or 4 tile columns, and
// inside a tile column a row is a 16-byte ALIGNED piece, 8 consecutive rows share one line: ~18 lines per keypoint instead of 39 rows x 1.34.
// Four consecutive lanes fetch four consecutive image rows of ONE tile column, starting at a row that is a multiple of 4: 64 contiguous
// bytes, half a line, per quad of lanes (measured against one patch row's four tile columns per quad, and against a compacted list of
// 7 chunks per lane: DESIGN 9).  So the LDS image starts at image row (y - 18) & ~3: 40 rows at a 64-byte pitch, LDS column 0 = image
// column 16 * tc0.
#define OD_TP 64
#define OD_TROWS 40
#define OD_KP_LDS_T ((OD_TROWS * OD_TP) / 4)             // dwords per keypoint (the 31 x 48-byte un-blurred patch fits in front): 24.7 KB per workgroup with the tables
__global__ __launch_bounds__(OD_THREADS) void k_orient_desc_tiled(OrbParams P)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OD_THREADS / 16][OD_KP_LDS_T];
    __shared__ float4 pat_t[16 * 16];            // pat_t[t][l] = test 16*l + t as floats x0,y0,x1,y1
    __shared__ int od_hw[48];                   // od_hw[3 + r]: blur_hw of blurred patch row r = 0 .. 36 (dy = r - 18), -64 outside: no chunk is fetched there
    __shared__ uint32_t od_msk[16 * 8];          // od_msk[|v|][j]: bytes of columns -15+4j..-12+4j inside the circular patch
    const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, sub = lane >> 4;
    OD_PROF_BEGIN();
    OD_TABLES();
    if (tid < 48) { const int r = tid - 3, d = r < 18 ? 18 - r : r - 18; od_hw[tid] = (r >= 0 && r <= 36) ? P.blur_hw[d] : -64; }
    // un-blurred: the patch row of task l16 + 16 k, and with it the half-width of the circular patch (umax) in that row, does not depend on
    // the keypoint: it stays in registers; -64 = no such row, the intersection test below then always fails
    int uhw[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { const int i = l16 + 16 * k, r = (i * 43) >> 7, d = r < 15 ? 15 - r : r - 15; uhw[k] = i < 31 * 3 ? P.umax[d] : -64; }
    __syncthreads();
    OD_WORK_SPLIT();
    OdHead nx = {};
    if (fk < nframes_x) od_head_issue<true>(P, kb, xcd + 8 * fk, 4 * g, sub, nx);          // the first trip's head: the only one a wave waits for
    OD_T(10);
    while (fk < nframes_x) {
        OD_TRIP_HEAD(true);
        // ---- stage both patches (16 lanes per keypoint)
        const int uxs = (x - 15) & ~3, uoff = (x - 15) - uxs;        // un-blurred: cols x-15..x+15
        const int tc0 = (x - 18) >> 4, boff = (x - 18) & 15, yoff = (y - 18) & 3;         // blurred:    cols x-18..x+18 = tile columns tc0 .. tc0 + 2 or 3, LDS column 0 = image column 16 * tc0
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // previous keypoints' LDS reads are done
        // the 16 lanes sweep the patch rows in 16-byte chunks: un-blurred 3 per row at a dword-aligned start (6 per lane), blurred the 4
        // ALIGNED chunks of a row's tile columns, each one tile row = a 16-byte piece of one 128-byte line (10 per lane: the 40 rows from
        // (y - 18) & ~3 on, lane = (tile column l16 >> 2, row 4 k + (l16 & 3))); a chunk that lies wholly outside the circular patch / the
        // sampled disc of its row is not fetched.  All loads are issued before the first LDS store so that they are in flight together;
        // the blurred chunks wait in registers until the moments are done with the shared region
        uint4 br[10];
        uint32_t bmask = 0, umask = 0;
#pragma unroll
        for (int k = 0; k < 10; k++) br[k] = make_uint4(0, 0, 0, 0);
        int bhw[10];                                                 // half-width of the sampled disc in the lane's rows
#pragma unroll
        for (int k = 0; k < 10; k++) bhw[k] = od_hw[4 * k + (l16 & 3) - yoff + 3];
        uint4 ur[6];
        if (valid) {
            const uint8_t *uimg = h.uimg, *bimg = h.bimg;
            const int upitch = h.upitch, tiles_x = h.bgeom;
            const uint32_t urow = (uint32_t)(((y - 15) & 0xFFFF) * upitch);
            const int blo = 16 * (l16 >> 2) - 18 - boff;                                  // patch columns blo .. blo + 15: the lane's tile column
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;      // i / 3 for i < 128
                const int ulo = 16 * c3 - 15 - uoff;                                 // patch columns ulo .. ulo + 15
                const bool on = ulo <= uhw[k] && ulo + 15 >= -uhw[k];
                ur[k] = on ? od_load16(uimg, urow + (uint32_t)(r * upitch), uxs + 16 * c3) : make_uint4(0, 0, 0, 0);
                umask |= on ? 1u << k : 0u;
            }
#pragma unroll
            for (int k = 0; k < 10; k++) {
                const int gy = y - 18 - yoff + (l16 & 3) + 4 * k;                   // image row of LDS row 4 k + (l16 & 3)
                if (blo <= bhw[k] && blo + 15 >= -bhw[k]) {                         // the chunk holds a column some angle samples: inside the image
                    br[k] = *reinterpret_cast<const uint4 *>(bimg + ((((uint32_t)(gy >> 3) * (uint32_t)tiles_x + (uint32_t)(tc0 + (l16 >> 2))) << 7) + (uint32_t)((gy & 7) << 4)));
                    bmask |= 1u << k;
                }
            }
        }
        if (fk < nframes_x) od_head_issue<true>(P, kb, xcd + 8 * fk, 4 * g, sub, nx);      // the next trip's head travels with this trip's patches
        OD_T(1); OD_VMWAIT(); OD_T(2);
#pragma unroll
        for (int k = 0; k < 6; k++) {                                                // umask == 0 for a slot without keypoint
            const int i = l16 + 16 * k, r = (i * 43) >> 7, c3 = i - r * 3;          // i / 3 for i < 128
            if (umask & (1u << k)) *reinterpret_cast<uint4 *>(&up32[r * (OD_UP / 4) + 4 * c3]) = ur[k];         // the others hold no byte od_msk keeps
        }
        wave_lds_sync();
        // ---- IC_Angle (ORBextractor.cc:75-102)
        OD_MOMENTS();
        OD_T(3);
        // the moments' LDS reads are done: the blurred patch takes the region over
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 10; k++)                                                // bmask == 0 for a slot without keypoint
            if (bmask & (1u << k)) *reinterpret_cast<uint4 *>(&bp32[((l16 & 3) + 4 * k) * (OD_TP / 4) + 4 * (l16 >> 2)]) = br[k];
        m10 = row16_allreduce_add_dpp(m10); m01 = row16_allreduce_add_dpp(m01);        // the keypoint's 16 lanes = one DPP row
        const float angle = fast_atan2_deg((float)m01, (float)m10);
        // ---- steered BRIEF on the blurred level (ORBextractor.cc:106-145)
        double sd, cd;
        sincos_det((double)__fmul_rn(angle, factor_pi), &sd, &cd);
        const float a = (float)cd, b = (float)sd;
        OD_T(4);
        wave_lds_sync();
        const uint32_t offk = (uint32_t)((18 + yoff) * OD_TP + boff + 18) - 65u * 0x4B400000u;      // row * 64 + col: the patch centre less the 65 K excess
        OD_BRIEF(OD_ROW64);
        OD_STORE();
        OD_T(5);
    }
    OD_PROF_END();
}

int orb_orient_desc_blocks(const OrbParams &P)
{
    // one group of 4 keypoint slots per wave and trip; enough workgroups that a wave makes few trips (in-order dispatch keeps the
    // set of patches in flight spatially tight: 4096 x 8 workgroups 0.58 ms vs 0.72 ms with 256 x 8 persistent ones at batch 1024;
    // with the head carried from trip to trip the step is the same at 4096, 2048 and 1024 x 8 and 0.03 / 0.13 ms slower at 512 / 256 x 8),
    // no more than the busiest XCD needs (small batches), the same number on every XCD.  desc_blocks_cap (ORBHIP_TUNE_DESC_BLOCKS=n when
    // the extractor reserved) caps the workgroups per XCD: a small batch then runs waves of many trips (tests), and the note can be re-measured
    const long groups_x = (long)((P.batch + 7) / 8) * ((P.kps_per_frame + 3) >> 2);      // frames are pinned to XCDs: work per XCD
    long blocks_x = (groups_x + (OD_THREADS / 64) - 1) / (OD_THREADS / 64);
    if (blocks_x > 4096) blocks_x = 4096;
    if (P.desc_blocks_cap > 0 && blocks_x > P.desc_blocks_cap) blocks_x = P.desc_blocks_cap;
    return (int)blocks_x;
}

void orb_launch_orient_desc(const OrbParams &P, hipStream_t s)
{
    const long blocks = 8 * (long)orb_orient_desc_blocks(P);
    if (P.blur_tiled) hipLaunchKernelGGL(k_orient_desc_tiled, dim3((unsigned)blocks), dim3(OD_THREADS), 0, s, P);
    else hipLaunchKernelGGL(k_orient_desc, dim3((unsigned)blocks), dim3(OD_THREADS), 0, s, P);
}

