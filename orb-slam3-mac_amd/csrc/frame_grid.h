// frame_grid.h -- the Frame grid (reference include/Frame.h:38-39, src/Frame.cc:377-408) as the windowed searches build it in LDS.
// Included by search_init_kernels.hip (the grid's size), match_kernels.hip (SearchByProjection, Fuse) and frame_kernels.hip (AssignFeaturesToGrid).  Force-inlined device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/orbhip.h"
#include "wave_dpp.h"

#define SI_COLS 64            // FRAME_GRID_COLS (include/Frame.h:38)
#define SI_ROWS 48            // FRAME_GRID_ROWS (include/Frame.h:39)
#define SBP_CELLS (SI_COLS * SI_ROWS)
struct OrbLevelSigma { float inv_sigma2[16]; };       // mvInvLevelSigma2, passed by value

// Frame::AssignFeaturesToGrid (Frame.cc:377-408) as a CSR in LDS, built by one wave: cell by round() (PosInGrid, :716-726),
// insertion order = index order.  rank = number of earlier keypoints in the same cell = the cell's counter before this trip +
// the earlier lanes of the trip with the same cell.  cell_start must be zeroed by the caller; on return cell_start[c] is the
// first slot of cell c = ix*48+iy in items[], and kx / ky / oct hold the keypoints' coordinates and octaves.
// Rig frames (Nleft != -1, Frame.cc:395-405): keypoints nleft .. n-1 are the right camera's and fill mGridRight, here the cells
// SBP_CELLS .. 2*SBP_CELLS-1 of the same CSR (ncells = 2*SBP_CELLS); items hold frame-wide indices (i = right index + Nleft).
__device__ __forceinline__ void sbp_build_grid(uint32_t *cell_start, float *kx, float *ky, uint8_t *oct, uint16_t *items, uint16_t *cell_of,
                                               uint16_t *rank_of, const orbhip_keypoint *kp, int n, float min_x, float min_y, float inv_w, float inv_h,
                                               int lane, int ncells = SI_COLS * SI_ROWS, int nleft = -1)
{
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        int c = 0xFFFF;
        if (i < n) {
            const orbhip_keypoint k = kp[i];
            kx[i] = k.x; ky[i] = k.y; oct[i] = (uint8_t)k.octave;
            const int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, min_x), inv_w));
            const int py = (int)roundf(__fmul_rn(__fsub_rn(k.y, min_y), inv_h));
            if (px >= 0 && px < SI_COLS && py >= 0 && py < SI_ROWS) c = px * SI_ROWS + py + ((nleft >= 0 && i >= nleft) ? SI_COLS * SI_ROWS : 0);
        }
        int intra = 0;
        for (int l = 0; l < 64; l++) {
            const int cl = __builtin_amdgcn_readlane(c, l);
            intra += (cl == c && l < lane);
        }
        if (i < n) {
            cell_of[i] = (uint16_t)c;
            if (c != 0xFFFF) rank_of[i] = (uint16_t)(cell_start[c + 1] + intra);
        }
        __syncthreads();                                          // every lane has read its counter
        if (i < n && c != 0xFFFF) atomicAdd(&cell_start[c + 1], 1u);
        __syncthreads();
    }
    {   // exclusive prefix over the cell counts (cell_start[c+1] holds count(c))
        uint32_t carry = 0;
        for (int c0 = 1; c0 <= ncells; c0 += 64) {
            const int c = c0 + lane;
            const int v = c <= ncells ? (int)cell_start[c] : 0;
            const int inc = wave_scan_add_dpp(v);
            if (c <= ncells) cell_start[c] = carry + (uint32_t)inc;
            carry += (uint32_t)__builtin_amdgcn_readlane(inc, 63);
        }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) { const int c = cell_of[i]; if (c != 0xFFFF) items[cell_start[c] + rank_of[i]] = (uint16_t)i; }
    __syncthreads();
}
