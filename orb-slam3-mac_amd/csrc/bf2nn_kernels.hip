// bf2nn_kernels.hip -- ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:2353-2369) and the all-pairs 2-NN + ratio test of
// Frame::ComputeStereoFishEyeMatches (src/Frame.cc:43,1146-1153: cv::BFMatcher knnMatch k = 2), as xor + popcount and on the matrix
// cores.  The only matcher file built with -amdgpu-mfma-vgpr-form (Makefile): k_bf2nn_mfma reads its accumulators right after the last MFMA.
#include "orb_internal.h"
#include "ctx_internal.h"
#include <climits>
#include <cstdlib>
#include <cstring>
#include <type_traits>

// host-callable scalar; same SWAR sequence as the reference (== sum of popcount32).
extern "C" int orbhip_descriptor_distance(const uint8_t *a32, const uint8_t *b32)
{
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t pa, pb;
        memcpy(&pa, a32 + 4 * i, 4); memcpy(&pb, b32 + 4 * i, 4);
        uint32_t v = pa ^ pb;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}

// ---------------------------------------------------------------------------- all-pairs 2-NN + ratio
// grid = (ceil(max_n/256), pairs); one query per thread; train tile of 256 descriptors in LDS.
// MONO (Frame::ComputeStereoFishEyeMatches, Frame.cc:1130-1134): pair p matches only rows [monoA[p], nA[p]) against [monoB[p], nB[p]) --
// the lapping slices -- and the row / train indices are slice-relative (knnMatch on rowRange(mono, rows)).  A pair whose counts exceed
// max_n writes nothing (the caller's triangulation kernel reports it).
#define BF_TILE 256
__device__ __forceinline__ bool bf_slice(const int32_t *nA, const int32_t *nB, const int32_t *monoA, const int32_t *monoB, int pair, int max_n,
                                         int &na, int &nb, int &ma, int &mb)
{
    na = nA[pair]; nb = nB[pair]; ma = 0; mb = 0;
    if (!monoA) return true;
    if (na > max_n || nb > max_n) return false;
    ma = min(max(monoA[pair], 0), max(na, 0)); mb = min(max(monoB[pair], 0), max(nb, 0));
    na -= ma; nb -= mb;
    return true;
}
template <bool MONO>
__global__ __launch_bounds__(256) void k_bf2nn(const uint8_t *descA, const int32_t *nA, size_t strideA,
                                               const uint8_t *descB, const int32_t *nB, size_t strideB,
                                               int max_n, double ratio, int32_t *idx2, int32_t *dist2, uint8_t *accept,
                                               const int32_t *monoA, const int32_t *monoB)
{
    __shared__ uint4 tile[BF_TILE * 2];
    const int pair = blockIdx.y, tid = threadIdx.x;
    int na, nb, ma, mb;
    if (!bf_slice(nA, nB, MONO ? monoA : nullptr, monoB, pair, max_n, na, nb, ma, mb)) return;
    const int q = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= na) return;
    const uint4 *A = reinterpret_cast<const uint4 *>(descA + (size_t)pair * strideA) + 2 * (size_t)ma;
    const uint4 *B = reinterpret_cast<const uint4 *>(descB + (size_t)pair * strideB) + 2 * (size_t)mb;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (q < na) { a0 = A[2 * q]; a1 = A[2 * q + 1]; }
    // best / second-best as keys (distance << 16 | train index): "first candidate wins on equal distance"
    // (strict < in the reference loop) is exactly the lexicographic order of the keys, so the running pair is
    // the two smallest keys -- three min/max per candidate instead of a compare-and-swap ladder
    uint32_t kb = 0xFFFFFFFFu, ks = 0xFFFFFFFFu;
    for (int t0 = 0; t0 < nb; t0 += BF_TILE) {
        const int tn = min(BF_TILE, nb - t0);
        __syncthreads();
        for (int i = tid; i < tn * 2; i += 256) tile[i] = B[2 * t0 + i];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < tn; j++) {
            const uint32_t key = ((uint32_t)hamming256(a0, a1, tile[2 * j], tile[2 * j + 1]) << 16) | (uint32_t)(t0 + j);
            ks = min(ks, max(kb, key));
            kb = min(kb, key);
        }
    }
    if (q < na) {
        const int best = kb == 0xFFFFFFFFu ? INT_MAX : (int)(kb >> 16), second = ks == 0xFFFFFFFFu ? INT_MAX : (int)(ks >> 16);
        const int bi = kb == 0xFFFFFFFFu ? -1 : (int)(kb & 0xFFFFu), si = ks == 0xFFFFFFFFu ? -1 : (int)(ks & 0xFFFFu);
        const size_t o = ((size_t)pair * max_n + q) * 2;
        idx2[o] = bi; idx2[o + 1] = si; dist2[o] = best; dist2[o + 1] = second;
        // Frame.cc:1153: (*it).size() >= 2 && (*it)[0].distance < (*it)[1].distance * 0.7  (float < float*double)
        accept[(size_t)pair * max_n + q] = (si >= 0 && (double)(float)best < (double)(float)second * ratio) ? 1 : 0;
    }
}

// The same 2-NN search on the matrix cores.  With the query bits widened to -1 / +1 bytes (a' = 1 - 2a) and the train bits to 0 / 1 bytes (b),
// <a', b> = |b| - 2 <a, b>, so Hamming(a, b) = |a| + |b| - 2 <a, b> = |a| + <a', b>: v_mfma_i32_32x32x32_i8 leaves the Hamming distance
// less the row's constant |a| in the accumulator (exact integers) and a key ordered like (distance << 16 | train index) is ONE
// v_lshl_add_u32 away; |a| is added once per row at the end.
// Descriptor matching is VALU-bound as xor + popcount (~21 vector instructions per pair and lane); here a 32 x 32 block of pairs costs
// 8 MFMAs plus 3 vector instructions per pair (key, v_med3 / v_min for the two smallest), issued between the MFMAs of the next block
// (the main loop below).  One workgroup = 8 waves
// x 32 queries of one pair of frames; the train side streams through LDS in tiles of 64 descriptors, widened once per workgroup
// (nibble * 0x00204081 & 0x01010101 puts 4 bits into 4 bytes), the next tile's fetch in flight behind this tile's MFMAs.
// A operand: lane l = (row l & 31, half l >> 5) holds bits [32 m + 16 h, +16) of its query for MFMA m; B likewise per train column, so
// element (h, j) of both operands is the same bit (the contraction index), whatever k the hardware assigns to it.  C: col = l & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Keys keep the reference's first-wins tie rule (cv::BFMatcher order).
#define BFM_ROWB 272                     // bytes per widened train descriptor in LDS (256 + 16: a 16-lane b128 read covers all banks once)
typedef int bfm_v4i __attribute__((ext_vector_type(4)));
typedef int bfm_v16i __attribute__((ext_vector_type(16)));
__device__ __forceinline__ uint32_t bfm_widen4(uint32_t nib) { return __umul24(nib, 0x00204081u) & 0x01010101u; }      // full-rate 24-bit multiply (nib < 16, constant < 2^22)
__device__ __forceinline__ uint32_t bfm_widen4_pm(uint32_t nib)          // 4 bits -> 4 bytes: bit 1 -> -1, bit 0 -> +1
{
    const uint32_t s = bfm_widen4(nib);                                    // bytes 0 / 1; s * 255 = bytes 0x00 / 0xFF (no carries), | 1 -> 0x01 / 0xFF
    return ((s << 8) - s) | 0x01010101u;
}
#define BFM_WAVES 8                      // waves (x 32 queries) per workgroup: the train tiles are widened once per workgroup
// four waves per SIMD (128 registers): two of this kernel's waves fit a SIMD beside one 234-register wave of k_search_init (the bench step)
template <bool MONO>
__global__ __launch_bounds__(64 * BFM_WAVES, 4) void k_bf2nn_mfma(const uint8_t *descA, const int32_t *nA, size_t strideA,
                                                    const uint8_t *descB, const int32_t *nB, size_t strideB,
                                                    int max_n, double ratio, int32_t *idx2, int32_t *dist2, uint8_t *accept,
                                                    const int32_t *monoA, const int32_t *monoB)
{
    __shared__ __attribute__((aligned(16))) uint8_t Bx[2 * 64 * BFM_ROWB];                 // two tile buffers of 64 x BFM_ROWB bytes (34 KB); at the end the merge area
    static_assert(BFM_WAVES * 2 * 8 * 64 * 4 <= 2 * 64 * BFM_ROWB, "the merge area (half of the rows at a time) fits the tile buffers");
    const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int na, nb, ma, mb;
    if (!bf_slice(nA, nB, MONO ? monoA : nullptr, monoB, pair, max_n, na, nb, ma, mb)) return;
    const int q0 = blockIdx.x * (32 * BFM_WAVES);
    if (q0 >= na) return;
    const uint32_t *A = reinterpret_cast<const uint32_t *>(descA + (size_t)pair * strideA) + 8 * (size_t)ma;
    const uint32_t *B = reinterpret_cast<const uint32_t *>(descB + (size_t)pair * strideB) + 8 * (size_t)mb;
    const int r = lane & 31, h = lane >> 5;
    // ---- the wave's 32 queries: operand fragments (8 MFMAs x 16 bytes of -1 / +1) and |a|
    const int qrow = q0 + 32 * wave + r;
    bfm_v4i af[8];
    int pa_row = 0;
    {
        uint32_t w[8];
#pragma unroll
        for (int m = 0; m < 8; m++) { w[m] = qrow < na ? A[(size_t)8 * qrow + m] : 0u; pa_row += __popc(w[m]); }
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t hw = (w[m] >> (16 * h)) & 0xFFFFu;
            af[m] = (bfm_v4i){(int)bfm_widen4_pm(hw & 15u), (int)bfm_widen4_pm((hw >> 4) & 15u), (int)bfm_widen4_pm((hw >> 8) & 15u), (int)bfm_widen4_pm(hw >> 12)};
        }
        asm volatile("" : "+v"(pa_row));          // summed here: left to the compiler the sum sinks to its use at the end and the 8 words stay in registers through the loop
    }
    // The chains start from C = 0 (an inline constant, no registers), so an accumulator holds <a', b> = Hamming - |a| in [-256, 256].  The
    // keys are ((acc + 256) << 16) + column: within one row |a| is a constant, so the two smallest keys are the two nearest columns, ties
    // to the lower column, exactly as with the distance itself; the merge at the end adds |a| - 256 to the row's two distances.
    uint32_t k1[16], k2[16];
#pragma unroll
    for (int g = 0; g < 16; g++) { k1[g] = 0xFFFFFFFFu; k2[g] = 0xFFFFFFFFu; }
    // ---- tiles of 64 train descriptors: thread t fetches dword t & 7 of descriptor t >> 3; the fetch of the NEXT tile is issued before
    //      this tile's MFMAs and widened into the other LDS buffer after them (its latency hides behind them)
    const int sc = tid >> 3, sm = tid & 7;
    auto fetch = [&](int t0, uint32_t &w0) { w0 = (t0 + sc < nb) ? B[(uint32_t)(8 * (t0 + sc) + sm)] : 0u; };      // nb <= 65535: a 32-bit offset
    auto widen = [&](int bufi, uint32_t w) {
        uint4 lo = make_uint4(bfm_widen4(w & 15u), bfm_widen4((w >> 4) & 15u), bfm_widen4((w >> 8) & 15u), bfm_widen4((w >> 12) & 15u));
        uint4 hi = make_uint4(bfm_widen4((w >> 16) & 15u), bfm_widen4((w >> 20) & 15u), bfm_widen4((w >> 24) & 15u), bfm_widen4(w >> 28));
        uint4 *dst = reinterpret_cast<uint4 *>(&Bx[bufi * 64 * BFM_ROWB + sc * BFM_ROWB + sm * 32]);
        dst[0] = lo; dst[1] = hi;
    };
    uint32_t nw0;
    fetch(0, nw0);
    widen(0, nw0);
    __syncthreads();
    // ---- the main loop is software-pipelined inside the wave over half tiles of 32 columns, with two accumulators in ping-pong: accA takes
    //      the first half of every tile, accB the second, and the 8 MFMAs of one half tile are issued between the 48 vector instructions
    //      (16 x key, v_med3, v_min) that retire the other accumulator -- two rows of keys per MFMA, so that the matrix pipe and the vector
    //      pipe work side by side and the last MFMA's wait states pass behind the other chain.  The B fragments come out of LDS through a
    //      ring of four quads, read four MFMAs ahead (the first four of a tile behind the first retired rows: a tile is readable only after
    //      its barrier).  The first reader of an accumulator element is the plain-C key (the hazard recogniser places the MFMA -> VALU wait
    //      states; an inline-asm first reader would not get them).  A column beyond the frame carries 0x40000000 in its keys, a value no
    //      descriptor's key reaches (bit 30: recognised at the end).  __builtin_amdgcn_sched_barrier(0) behind every MFMA's group keeps the
    //      interleave as written (sched_group_barrier's masks do not see the asm statement with v_med3 / v_min).
    const bfm_v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bfm_v16i accA = zero, accB = zero;
    uint32_t baseB = 0;
    auto retire = [&](const bfm_v16i &acc, uint32_t base, int g) {
        const uint32_t key = ((uint32_t)acc[g] << 16) + base;
        asm("v_med3_u32 %1, %0, %2, %1\n\tv_min_u32 %0, %0, %2" : "+v"(k1[g]), "+v"(k2[g]) : "v"(key));      // k1 <= k2: the middle one is the new second best
    };
    auto key_base = [&](int col) { return (col < nb ? (uint32_t)col : (0x40000000u | (uint32_t)col)) + (256u << 16); };
    const uint8_t *bx0 = &Bx[r * BFM_ROWB + h * 16];
    int buf = 0, t0 = 0;
    auto tile = [&](auto first) {                                             // a tile with both halves; the first one has nothing to retire yet
        constexpr bool FIRST = decltype(first)::value;
        const bool more = t0 + 64 < nb;
        if (more) fetch(t0 + 64, nw0);
        const uint8_t *bx = bx0 + buf * 64 * BFM_ROWB;
        auto rd = [&](int q) { return *reinterpret_cast<const bfm_v4i *>(bx + (q >> 3) * 32 * BFM_ROWB + (q & 7) * 32); };      // quad q = 8 * half + MFMA
        bfm_v4i bq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) bq[q] = rd(q);
        if constexpr (!FIRST) {
#pragma unroll
            for (int g = 0; g < 4; g++) retire(accB, baseB, g);               // these cover the LDS round trip of the first quads
        }
        const uint32_t baseA = key_base(t0 + r);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            accA = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[m], bq[m & 3], m ? accA : zero, 0, 0, 0);
            bq[m & 3] = rd(m + 4);
            if constexpr (!FIRST) {
                retire(accB, baseB, 4 + 3 * (m >> 1) + 2 * (m & 1));
                if (!(m & 1)) retire(accB, baseB, 5 + 3 * (m >> 1));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        baseB = key_base(t0 + 32 + r);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            accB = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[m], bq[m & 3], m ? accB : zero, 0, 0, 0);
            if (m < 4) bq[m & 3] = rd(m + 12);
            if (m) {                                                          // 16 rows behind MFMAs 1..7 (2, 2, 3, 2, 2, 3, 2): accA's wait states pass behind MFMA 0
                const int g0 = (16 * (m - 1) + 6) / 7, g1 = (16 * m + 6) / 7;
#pragma unroll
                for (int g = g0; g < g1; g++) retire(accA, baseA, g);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) widen(buf ^ 1, nw0);
        __syncthreads();
        t0 += 64; buf ^= 1;
    };
    if (32 < nb) tile(std::true_type());
    while (t0 + 32 < nb) tile(std::false_type());
    if (t0 < nb) {                                                            // uniform: a last tile of one half; nothing is left to issue behind it
        const uint8_t *bx = bx0 + buf * 64 * BFM_ROWB;
        bfm_v4i bq[8];
#pragma unroll
        for (int m = 0; m < 8; m++) bq[m] = *reinterpret_cast<const bfm_v4i *>(bx + m * 32);
#pragma unroll
        for (int m = 0; m < 8; m++) accA = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[m], bq[m], m ? accA : zero, 0, 0, 0);
        if (t0) {                                                             // the half tile before it is still in accB
#pragma unroll
            for (int g = 0; g < 16; g++) retire(accB, baseB, g);
        }
        const uint32_t baseA = key_base(t0 + r);
#pragma unroll
        for (int g = 0; g < 16; g++) retire(accA, baseA, g);
        __syncthreads();                                                      // the merge below reuses the tile buffers
    } else if (nb > 0) {                                                      // the last half tile is still in accB
#pragma unroll
        for (int g = 0; g < 16; g++) retire(accB, baseB, g);
    }
    // ---- merge the 32 columns (lanes of one half) of every row: through LDS (the tile buffers are free now), four lanes per row with 8 columns
    //      each (every lane starts at another column: 2 lanes per bank instead of 16), then two exchange steps among the four; rows 0..15
    //      (accumulator registers 0..7) first, then rows 16..31, so that the area is 32 KB and the kernel's LDS stays at the 34 KB of its
    //      tile buffers (64 KB until round 4: two workgroups filled 128 KB of a CU and no other kernel's workgroup could start beside them)
    uint32_t (*kout)[2][8][64] = reinterpret_cast<uint32_t (*)[2][8][64]>(&Bx[0]);           // [wave][k1 | k2][reg & 7][lane]
#pragma unroll
    for (int part = 0; part < 2; part++) {
        if (part) __syncthreads();
#pragma unroll
        for (int g = 0; g < 8; g++) { kout[wave][0][g][lane] = k1[8 * part + g]; kout[wave][1][g][lane] = k2[8 * part + g]; }
        __syncthreads();
        const int row = 16 * part + (lane >> 2), g = (row & 3) + 4 * ((row >> 3) & 1), hh = (row >> 2) & 1;
        const int unbias = __shfl(pa_row, row, 64) - 256;                      // |a| of the row this lane merges (lanes 0..31 hold rows 0..31)
        uint32_t kb = 0xFFFFFFFFu, ks = 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int cc = 32 * hh + 8 * (lane & 3) + ((c + (lane >> 2)) & 7);
            const uint32_t a1 = kout[wave][0][g][cc], a2 = kout[wave][1][g][cc];
            ks = min(min(ks, a2), max(kb, a1));                                    // two smallest of {kb, ks, a1, a2} (a1 <= a2, kb <= ks)
            kb = min(kb, a1);
        }
#pragma unroll
        for (int s = 1; s < 4; s <<= 1) {
            const uint32_t pb = __shfl_xor(kb, s, 64), ps = __shfl_xor(ks, s, 64);
            ks = min(min(ks, ps), max(kb, pb));
            kb = min(kb, pb);
        }
        const int q = q0 + 32 * wave + row;
        if ((lane & 3) == 0 && q < na) {
            const bool hb = !(kb & 0x40000000u), hs = !(ks & 0x40000000u);              // a real column (else: no such neighbour)
            const int best = hb ? (int)(kb >> 16) + unbias : INT_MAX, second = hs ? (int)(ks >> 16) + unbias : INT_MAX;
            const int bi = hb ? (int)(kb & 0xFFFFu) : -1, si = hs ? (int)(ks & 0xFFFFu) : -1;
            const size_t o = ((size_t)pair * max_n + q) * 2;
            idx2[o] = bi; idx2[o + 1] = si; dist2[o] = best; dist2[o + 1] = second;
            accept[(size_t)pair * max_n + q] = (si >= 0 && (double)(float)best < (double)(float)second * ratio) ? 1 : 0;
        }
    }
}

extern "C" int orbhip_match_bf2nn_device(orbhip_ctx *ctx, const uint8_t *d_descA, const int32_t *d_nA, size_t strideA,
                                         const uint8_t *d_descB, const int32_t *d_nB, size_t strideB, int pairs,
                                         int max_n, double ratio, int32_t *d_idx2, int32_t *d_dist2, uint8_t *d_accept)
{
    if (!ctx || !d_descA || !d_descB || !d_nA || !d_nB || pairs <= 0 || max_n <= 0 || max_n > 65535 || !d_idx2 || !d_dist2 || !d_accept)
        return ORBHIP_E_BADARG;              // train indices ride in 16 bits of the 2-NN keys
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    if (max_n >= 64 && !getenv("ORBHIP_BF2NN_VALU")) {          // matrix-core form (the xor / popcount kernel stays for tiny frames and as a cross-check)
        dim3 grid((max_n + 32 * BFM_WAVES - 1) / (32 * BFM_WAVES), pairs);
        hipLaunchKernelGGL(k_bf2nn_mfma<false>, grid, dim3(64 * BFM_WAVES), 0, orbhip_ctx_stream_internal(ctx), d_descA, d_nA, strideA, d_descB, d_nB,
                           strideB, max_n, ratio, d_idx2, d_dist2, d_accept, nullptr, nullptr);
    } else {
        dim3 grid((max_n + 255) / 256, pairs);
        hipLaunchKernelGGL(k_bf2nn<false>, grid, dim3(256), 0, orbhip_ctx_stream_internal(ctx), d_descA, d_nA, strideA, d_descB, d_nB,
                           strideB, max_n, ratio, d_idx2, d_dist2, d_accept, nullptr, nullptr);
    }
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

// The same search on the lapping slices [d_monoA[p], d_nA[p]) x [d_monoB[p], d_nB[p]) (orbhip_compute_stereo_fisheye_matches_device):
// same kernel choice; outputs at [p * max_n + slice row], train indices slice-relative.  Caller has checked the arguments.
int orbhip_bf2nn_slices_internal(orbhip_ctx *ctx, const uint8_t *d_descA, const int32_t *d_nA, const int32_t *d_monoA, size_t strideA,
                                 const uint8_t *d_descB, const int32_t *d_nB, const int32_t *d_monoB, size_t strideB, int pairs, int max_n,
                                 double ratio, int32_t *d_idx2, int32_t *d_dist2, uint8_t *d_accept)
{
    if (max_n >= 64 && !getenv("ORBHIP_BF2NN_VALU")) {
        dim3 grid((max_n + 32 * BFM_WAVES - 1) / (32 * BFM_WAVES), pairs);
        hipLaunchKernelGGL(k_bf2nn_mfma<true>, grid, dim3(64 * BFM_WAVES), 0, orbhip_ctx_stream_internal(ctx), d_descA, d_nA, strideA, d_descB, d_nB,
                           strideB, max_n, ratio, d_idx2, d_dist2, d_accept, d_monoA, d_monoB);
    } else {
        dim3 grid((max_n + 255) / 256, pairs);
        hipLaunchKernelGGL(k_bf2nn<true>, grid, dim3(256), 0, orbhip_ctx_stream_internal(ctx), d_descA, d_nA, strideA, d_descB, d_nB,
                           strideB, max_n, ratio, d_idx2, d_dist2, d_accept, d_monoA, d_monoB);
    }
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}
