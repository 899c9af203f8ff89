// Internal structures shared by the ORB kernels and the C-ABI implementation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/orbhip.h"

#define ORB_MAX_LEVELS 16
#define ORB_EDGE 19           // EDGE_THRESHOLD  (ORBextractor.cc:72)
#define ORB_MINB 16           // minBorder = EDGE_THRESHOLD-3 (ORBextractor.cc:771)
#define ORB_HALF_PATCH 15
#define ORB_RS_STEPS 24       // k_resize_rows: source-row steps per band (tests/test_gpu_orb_row_schedule.py carries a copy, RS_STEPS, and a
                              // mirror of the band rule of orb_plan_resize (pyramid_kernels.hip), which it asserts against orbhip_extractor_resize_band_rows)

// One pyramid level, batched: frame f lives at img + f*frame_stride, rows at pitch.
struct OrbLevel {
    uint8_t *img;             // un-padded level image (level 0 may alias the caller's input)
    uint8_t *blur;            // 7x7 sigma-2 blurred level
    size_t img_frame_stride;
    size_t blur_frame_stride;
    int w, h, img_pitch, blur_pitch;
    int blur_tiles_x;         // tiled blurred level (OrbParams::blur_tiled): 16 x 8-pixel tiles per tile row, (w + 15) / 16
    // FAST cell grid (ORBextractor.cc:774-781)
    int ncols, nrows, wcell, hcell;
    int cell_base;            // first cell of this level in the per-frame cell array
    int cell_cap;             // entries per cell list
    // octree
    int quota;                // mnFeaturesPerLevel[level]
    int key_base, key_cap;    // ordered-candidate scratch slice (per frame)
    int kp_base, kp_cap;      // per-level keypoint staging slice (per frame)
    int n_ini;                // nIni (ORBextractor.cc:541)
    float hx;                 // hX   (ORBextractor.cc:543)
    float scale;              // mvScaleFactor[level]
    float size;               // (int)(PATCH_SIZE*scale) as float (ORBextractor.cc:862)
    // resize tables (device): xofs[w], xalpha[2w], yofs[h], ybeta[2h]  (level>0)
    const int16_t *xofs; const int16_t *xalpha; const int16_t *yofs; const int16_t *ybeta;
    // k_resize_rows tables (level>0; xchunk == nullptr: the source span of 4 output columns does not fit 8 bytes, k_resize is used):
    // xchunk[12 * c] = {load offset, sel[4], alpha[4], v_perm selector of the byte shift, 0, 0} per 4 output columns,
    // ytab[band * ORB_RS_STEPS + i] = {source row, emit, b0 << 12, b1 << 12}: step i of the band's walk down its source rows (rs_rows output rows per band)
    const uint32_t *xchunk; const uint32_t *ytab;
    int resize_mode;          // k_resize_rows<MODE>: 0 unaligned 8-byte loads, 1 aligned dwordx3 + byte shift
    int rs_rows;              // k_resize_rows: output rows per band -- the most whose source rows fit ORB_RS_STEPS steps on every band of the level
};

struct OrbParams {
    OrbLevel lv[ORB_MAX_LEVELS];
    int nlevels, batch;
    int n_cus;                // compute units of the context's device
    int ini_th, min_th;
    int cells_per_frame;      // sum over levels of ncols*nrows
    int keys_per_frame;       // sum of key_cap
    int kps_per_frame;        // sum of kp_cap  (== staging slots per frame)
    int max_kp;               // output row capacity per frame
    int oct_nc;               // k_octree: node capacity of its LDS arrays = max over levels of max(quota + 16, 4*nIni + 4)
    int oct_dmax;             // k_octree_tab: depth of its deepest count table (orb_octree_dmax); 0: k_octree (the iterative form) runs instead
    int rows_min_batch;       // the row-streaming pyramid / blur kernels are used from this batch size on (below it the tile kernels have the shorter latency)
    int bm_min_batch;         // the matrix-core blur (k_blur_mfma) is used from this batch size on (its tables exist when bm_cols[nlevels] > 0)
    int br_blocks[ORB_MAX_LEVELS + 1];  // k_blur_rows: prefix of 256-lane workgroups per frame over the levels; [nlevels] == 0: k_blur (tiles) is used
    int bs_tiles[ORB_MAX_LEVELS + 1];   // k_blur: prefix of 64x32 tiles per frame over the levels (one launch for all levels)
    int desc_blocks_cap;      // > 0: at most that many workgroups per XCD in k_orient_desc (ORBHIP_TUNE_DESC_BLOCKS, read by reserve)
    int lap0, lap1;
    // per-frame scratch
    uint32_t *cell_count;     // [batch][cells_per_frame]
    uint32_t *cell_list;      // [batch][sum(cells*cell_cap)]  packed x | y<<12 | score<<24
    size_t cell_list_frame_stride;
    uint32_t *keys;           // [batch][keys_per_frame] ordered candidates (packed)
    uint16_t *node_of;        // [batch][keys_per_frame]
    uint32_t *lvl_kp;         // [batch][kps_per_frame] selected keypoints (packed)
#define ORB_PERM_MIN_BATCH 16   // below this batch size k_orient_desc keeps the slot order (single-frame latency)
    uint16_t *lvl_perm;       // [batch][kps_per_frame] per level: position (inside the level slice) of the r-th keypoint in spatial order -- the order
                              // k_orient_desc WORKS in (patches of neighbours share cache lines); results stay in the reference's slots
    uint32_t *lvl_wkey;       // [batch][kps_per_frame] per level: the selected keypoints (packed, as lvl_kp) in the spatial order, lvl_wkey[r] =
                              // lvl_kp[lvl_perm[r]] -- written with lvl_perm (batch >= ORB_PERM_MIN_BATCH), so k_orient_desc reads key and position with
                              // two independent loads; entries beyond the level's count are stale
    float *lvl_angle;         // [batch][kps_per_frame]
    uint8_t *lvl_desc;        // [batch][kps_per_frame][32]
    int32_t *lvl_count;       // [batch][nlevels]   post-octree count
    int32_t *lvl_ncand;       // [batch][nlevels]   pre-octree count
    int32_t *status;          // [1] sticky error flag (capacity overflow)
    // outputs
    orbhip_keypoint *out_kp;  // [batch][max_kp]
    uint8_t *out_desc;        // [batch][max_kp][32]
    int32_t *out_count;       // [batch]
    int32_t *out_mono;        // [batch]
    int umax[ORB_HALF_PATCH + 1];
    int gauss_q8[7];
    // k_blur_mfma (round 3): the 7x7 blur as two banded int8 matrix products per 64 x 64 window, one wave per 32-column tile column
    const uint4 *bm_th;                 // [tile columns of all levels][2 output blocks][64 lanes] horizontal band operands, image borders folded in
    const uint4 *bm_tv;                 // [4 output blocks][64 lanes] vertical band operands
    int bm_cols[ORB_MAX_LEVELS + 1];    // prefix of tile columns per frame over the levels; [nlevels] == 0: the kernel is not used
    int bm_init;                        // 128 * (sum of the taps): turns the biased int8 sums back into the plain ones
    // tiled blurred pyramid: the matrix-core blur writes, and k_orient_desc_tiled reads, the blurred levels in tiles of 16 px x 8 rows
    // (128 bytes = one cache line, row-major inside, tiles row-major in the level): byte (x, y) lives at ORB_BLUR_TILE_OFF(x, y, blur_tiles_x)
    int blur_tiled_ok;                  // reserve: the layout may be used (ORBHIP_BLUR_TILED=0 keeps every batch row-major)
    int blur_tiled;                     // per call: set exactly when orb_launch_blur takes k_blur_mfma
    int blur_hw[ORB_EDGE];              // blur_hw[|dy|]: the rBRIEF samples of patch row dy lie in columns [-blur_hw, blur_hw] for every angle
};

// k_fast_cells has its own, compact parameter block (scalar loads of per-level fields are what a persistent wave does most)
struct FcLevel {                  // (k_fast_runs only: k_fast_cells reads its geometry from the cell table)
    int max_bx, max_by;           // w - minBorder, h - minBorder
    int ncols, nrows, wcell, hcell, cell_base, cell_cap;
    int rpc, rpr, run_base;       // k_fast_runs: cells per run (2 while two cells fit 64 pixels, else 1), runs per cell row, first run of this level in a frame's run array
};
// A level's image as this call sees it (level 0 is the caller's buffer): the only per-level values k_fast_cells reads per cell
struct FcImage { const uint8_t *img; size_t frame_stride; int pitch, pad_; };
// k_fast_cells' cell table: one 16-byte record per cell of a frame, in the order the kernel walks them (level, then row-major), built once
// by orb_plan_fast -- everything of a cell that the image size fixes (ORBextractor.cc:783-806).  Packing (fc_rec_* below decode it, on
// the host and in the kernel):
//   xy   = x0 | y0 << 16                    first staged pixel (ini_x - 1, ini_y)
//   band = dw | dh << 6 | tpr << 12 | magic << 16     detection band (0 x 0: the reference skips the cell, :788, :797); lane layout of the
//                                           necessary test: two-pair tasks per row (nominal cell width, 8 .. 15) and magic = 65536 / tpr + 1,
//                                           floor(i / tpr) == (i * magic) >> 16 for i < 64; rows per trip = 64 / tpr = magic >> 10
//   key  = key_x0 | key_y0 << 12 | level << 24        the packed key (ORB_PACK_KEY) of band pixel (0, 0), score 0
//   list = cell * cell_cap                  the cell's list inside a frame's cell_list
struct FcRecord { uint32_t xy, band, key, list; };
__host__ __device__ __forceinline__ int fc_rec_x0(const FcRecord &r) { return (int)(r.xy & 0xFFFFu); }
__host__ __device__ __forceinline__ int fc_rec_y0(const FcRecord &r) { return (int)(r.xy >> 16); }
__host__ __device__ __forceinline__ int fc_rec_dw(const FcRecord &r) { return (int)(r.band & 63u); }
__host__ __device__ __forceinline__ int fc_rec_dh(const FcRecord &r) { return (int)((r.band >> 6) & 63u); }
__host__ __device__ __forceinline__ int fc_rec_tpr(const FcRecord &r) { return (int)((r.band >> 12) & 15u); }
__host__ __device__ __forceinline__ uint32_t fc_rec_magic(const FcRecord &r) { return r.band >> 16; }
__host__ __device__ __forceinline__ int fc_rec_rpt(const FcRecord &r) { return (int)(r.band >> 26); }
__host__ __device__ __forceinline__ uint32_t fc_rec_key0(const FcRecord &r) { return r.key & 0xFFFFFFu; }
__host__ __device__ __forceinline__ int fc_rec_level(const FcRecord &r) { return (int)(r.key >> 24); }
struct FastParams {
    FcLevel lv[ORB_MAX_LEVELS];
    FcImage im[ORB_MAX_LEVELS];   // set per call
    const FcRecord *cell_tab;     // [cells_per_frame], device copy of orb_plan_fast's table (uploaded by reserve)
    int nlevels, batch, ini_th, min_th, cells_per_frame;
    int cell_cap;                 // entries per cell list (the same on every level)
    int n_cus;                    // compute units of the context's device (hipDeviceAttributeMultiprocessorCount): sizes the persistent grid
    int chunk;                    // consecutive cells a wave takes at a time (set per launch)
    int lvl_lo, lvl_hi;           // this launch covers the cells of levels [lvl_lo, lvl_hi) of every frame (level 0 can start before the pyramid exists)
    // k_fast_cells, set per launch: the launch's cells of a frame are records [cell_lo, cell_hi) of the table; total = batch * (cell_hi - cell_lo)
    // cells in all; from the last cell of a chunk to the first of the wave's next one it is hop = hop_q * (cell_hi - cell_lo) + hop_r cells
    int cell_lo, cell_hi; uint32_t total, hop, hop_q, hop_r;
    uint32_t *cell_count, *cell_list; size_t cell_list_frame_stride; int32_t *status;
    // per-wave LDS geometry (from the largest cell of this extractor): pair tile [rows][PITCH] dwords, score tile [srows + 2][SPITCH]
    // dwords, queue of qcap u16; wave_dw = dwords per wave.  small_cells: every level fits the <28, 24, 9> instantiation
    int rows, srows, qcap, wave_dw, small_cells;
    // k_fast_runs (round 4): runs of up to two horizontally adjacent cells per wave
    int runs_per_frame, run_rows, run_q0, run_dw, use_runs;      // LDS rows of the pair tile, entries of the first queue, dwords per wave
};

#define ORB_BLUR_TILE_OFF(x, y, tiles_x) ((((uint32_t)((y) >> 3) * (uint32_t)(tiles_x) + (uint32_t)((x) >> 4)) << 7) + (uint32_t)(((y) & 7) << 4) + (uint32_t)((x) & 15))
#define ORB_PACK_KEY(x, y, s) ((uint32_t)(x) | ((uint32_t)(y) << 12) | ((uint32_t)(s) << 24))
#define ORB_KEY_X(k) ((int)((k) & 0xFFFu))
#define ORB_KEY_Y(k) ((int)(((k) >> 12) & 0xFFFu))
#define ORB_KEY_S(k) ((int)((k) >> 24))

// load types more than one stage file uses: three dwords at a 4-byte-aligned address (k_resize_rows<1>, k_blur_rows), four at any address
// (the FAST staging loads, k_blur_mfma)
typedef uint32_t rs_u32x3 __attribute__((ext_vector_type(3)));
typedef rs_u32x3 rs_u32x3_a4 __attribute__((aligned(4)));
struct __attribute__((packed, aligned(1))) u32x4_unaligned { uint32_t x, y, z, w; };

// Hamming distance of two 256-bit ORB descriptors held as two uint4 each (ORBmatcher::DescriptorDistance, ORBmatcher.cc:2353-2369):
// shared by the matcher files (bf2nn_ / search_init_ / match_ / bow_ / tri_kernels.hip) and stereo_kernels.hip
__device__ __forceinline__ int hamming256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Frame::ComputeStereoMatches (stereo_kernels.hip): the two extractors' pyramids and device outputs
struct StereoLevel {
    const uint8_t *imgL, *imgR;
    size_t fsL, fsR;              // frame strides
    int pitchL, pitchR, wR, pad_;
    float scale, inv_scale;       // mvScaleFactors / mvInvScaleFactors of the LEFT extractor
};
struct StereoArgs {
    StereoLevel lv[ORB_MAX_LEVELS];
    int nlevels, batch, max_kp, rows0;
    const orbhip_keypoint *kpL, *kpR;
    const uint8_t *descL, *descR;
    const int32_t *nL, *nR;
    float mb, mbf;
    float *u_right, *depth;
    int32_t *sad, *n_kept;
};
void orb_launch_stereo(const StereoArgs &A, hipStream_t s);

// Opt a kernel into the largest dynamic-LDS size a workgroup may have (160 KB minus its static LDS), once per (kernel, device);
// thread-safe, never lowers the limit again.  `need` = the dynamic bytes of the coming launch: more than the limit -> error.
int orb_lds_optin(const void *func, int device, size_t need);

// Host plans (no HIP call): each stage's file turns the extractor's geometry into the parameter fields and host tables of its own
// kernels; orbhip_extractor_reserve allocates, uploads and opts into LDS.
bool orb_plan_cell_grid(OrbLevel &L);                                                             // fast_kernels.hip: ncols .. hcell from w, h; false: no cell fits
void orb_plan_fast(const OrbParams &P, FastParams &F, std::vector<FcRecord> &cell_tab);           // fast_kernels.hip; upload cell_tab -> F.cell_tab
bool orb_plan_resize(OrbParams &P, int level, const std::vector<int16_t> &xofs, const std::vector<int16_t> &xalpha, const std::vector<int16_t> &yofs,
                     const std::vector<int16_t> &ybeta, std::vector<uint32_t> &xchunk, std::vector<uint32_t> &ytab);      // pyramid_kernels.hip; true: upload xchunk / ytab
bool orb_plan_blur(OrbParams &P, std::vector<int8_t> &bm_th, std::vector<int8_t> &bm_tv);         // blur_kernels.hip; true: upload bm_th / bm_tv
int orb_blur_kernel(const OrbParams &P, int batch);     // blur_kernels.hip: the kernel that blurs a batch of that size -- 0 k_blur (tiles), 1 k_blur_rows, 2 k_blur_mfma

// kernel launchers: pyramid_kernels.hip
void orb_launch_resize(const OrbParams &P, int level, hipStream_t s);
// fast_kernels.hip
// max_per_cu: 0 = as many waves as fit.  false: batch * cells does not fit the kernel's 32-bit cell counter, nothing was launched
bool orb_launch_fast_cells(const FastParams &F, hipStream_t s, int max_per_cu, int lvl_lo = 0, int lvl_hi = -1);
const void *orb_fast_runs_func(int nld);
int orb_fast_runs_nld(const FastParams &F);
int orb_fast_variant(const FastParams &F);
const void *orb_fast_cells_func(int small);
#define ORB_OVERLAP_MIN_BATCH 16
// blur_kernels.hip
#ifndef BLR_R
#define BLR_R 24              // k_blur_rows: output rows per lane (multiple of 6)
#endif
void orb_launch_blur(const OrbParams &P, hipStream_t s, int wgs_per_cu, int frame0 = 0, int nframes = -1);   // row kernel: frames [frame0, frame0 + nframes)
// desc_kernels.hip
void orb_launch_orient_desc(const OrbParams &P, hipStream_t s);
int orb_orient_desc_blocks(const OrbParams &P);   // workgroups (of two waves) per XCD of that launch
// orb_kernels.hip
void orb_launch_octree(const OrbParams &P, hipStream_t s, int parts = 3);
void orb_launch_assemble(const OrbParams &P, hipStream_t s);
size_t orb_octree_lds_bytes(int nc);
int orb_octree_nc(const OrbParams &P);
int orb_octree_dmax(const OrbParams &P);
const void *orb_octree_func(int which = 0);     // 0 k_octree, 1 k_octree_tab, 2 k_octree_redo
