// ctx_internal.h -- the context's internal interface: what the kernel files ask of an orbhip_ctx (orbhip_api.hip defines all of it and
// includes this header too, so a definition that drifts from its declaration fails to compile instead of linking wrong), the one
// cross-file launcher, and the host-side helpers every entry point uses.  Host code only.
#pragma once
#include "orb_internal.h"

hipStream_t orbhip_ctx_stream_internal(orbhip_ctx *c);
int orbhip_ctx_device_internal(orbhip_ctx *c);
int orbhip_ctx_cus_internal(orbhip_ctx *c);
int orbhip_ctx_ba_schur_mode_internal(orbhip_ctx *c);
int32_t *orbhip_ctx_status_internal(orbhip_ctx *c);                       // the sticky device-side error word (or its redirection)
void orbhip_ctx_redirect_status_internal(orbhip_ctx *c, int32_t *p);      // host_entry.hip: the word travels inside the call's blob; nullptr restores
// grow-only arenas, kept across calls; nullptr (and the last error set) when they cannot grow
void *orbhip_ctx_scratch_internal(orbhip_ctx *c, size_t bytes);           // device: staged inputs of the host-pointer entry points
void *orbhip_ctx_work_internal(orbhip_ctx *c, size_t bytes);              // device: the device entry points' own work buffers
void orbhip_ctx_note_sbp_redo_internal(orbhip_ctx *c, size_t offset, int pairs);   // match_kernels.hip: where in the work arena the last launch's hand-back flags lie
void *orbhip_ctx_pinned_internal(orbhip_ctx *c, size_t bytes);            // page-locked host
// one-shot local-BA solves: a cached device arena (nullptr: lent out already, or cannot grow) and one page-locked word
void *orbhip_ctx_ba_arena_acquire_internal(orbhip_ctx *c, size_t bytes);
void orbhip_ctx_ba_arena_release_internal(orbhip_ctx *c);
int *orbhip_ctx_pinned_word_internal(orbhip_ctx *c);
// what orbhip_last_error() returns next on this thread; `msg` must outlive the call (string literals)
void orbhip_set_last_error_internal(const char *msg);

// bf2nn_kernels.hip: the all-pairs 2-NN on the lapping slices [d_monoA[p], d_nA[p]) x [d_monoB[p], d_nB[p]) (tri_kernels.hip calls it)
int orbhip_bf2nn_slices_internal(orbhip_ctx *ctx, const uint8_t *d_descA, const int32_t *d_nA, const int32_t *d_monoA, size_t strideA,
                                 const uint8_t *d_descB, const int32_t *d_nB, const int32_t *d_monoB, size_t strideB, int pairs, int max_n,
                                 double ratio, int32_t *d_idx2, int32_t *d_dist2, uint8_t *d_accept);

// newpoints_kernels.hip: the checks on the HOST per-pair records, and the launch with the records already on the device (host_entry.hip
// carries them in its blob); arguments as orbhip_create_new_map_points_device
int orbhip_newpoints_check_internal(const orbhip_newpoints_pair *pair, int pairs, int max_n, int nlevels);
int orbhip_newpoints_launch_internal(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kp1, const orbhip_keypoint *d_kp1_raw, const float *d_u_right1, const float *d_depth1, const int32_t *d_n1,
        const orbhip_keypoint *d_kp2, const orbhip_keypoint *d_kp2_raw, const float *d_u_right2, const float *d_depth2, const int32_t *d_n2,
        const int32_t *d_matches12, const orbhip_newpoints_pair *d_pair, int pairs, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors1, const float *level_sigma2_2, const float *scale_factors2, int nlevels,
        uint8_t *d_has_mp1, uint8_t *d_has_mp2, float *d_x3D, uint8_t *d_outcome, int32_t *d_n_created);

// mlpnp_kernels.hip: the parameter and capacity rules of orbhip_mlpnp_solver_device / _host, each failure named by orbhip_last_error()
extern "C" int orbhip_mlpnp_check_params_internal(const orbhip_mlpnp_params *p, int max_n);

// frustum_kernels.hip: the checks on the HOST per-frame records, and the frustum kernel followed by the local-map matcher with the records
// already on the device (host_entry.hip carries them in its blob); arguments as orbhip_search_local_points_device
int orbhip_local_points_check_internal(const orbhip_frustum_frame *frame, int frames, int max_points, int max_q, bool rig_train, bool has_u_right,
                                       int max_n, size_t frame_stride_kp, float min_x, float min_y, float max_x, float max_y);
int orbhip_frustum_check_internal(const orbhip_frustum_frame *frame, int frames, int max_points, int max_q);
int orbhip_frustum_launch_internal(orbhip_ctx *ctx, const orbhip_frustum_frame *d_frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, float min_x, float min_y, float max_x, float max_y, int max_q,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq);
int orbhip_local_points_chain_internal(orbhip_ctx *ctx, const orbhip_frustum_frame *d_frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc_kp,
        const float *d_u_right, const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n, size_t frame_stride_kp,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq,
        int32_t *d_train_match, int32_t *d_nmatches);

// kfdb_kernels.hip: the argument checks and the kernel chain of orbhip_kfdb_score_device / _detect_device; d_query != nullptr: the query
// records are on the device already (host_entry.hip carries them in its blob) and `query` (HOST) is only checked
int orbhip_kfdb_launch_internal(orbhip_kfdb *db, const char *who, const orbhip_kfdb_query *query, const orbhip_kfdb_query *d_query, int queries,
        const int32_t *d_qword, const double *d_qvalue, const int32_t *d_qn, int q_stride, const int32_t *d_connected,
        const int32_t *d_nconnected, int max_connected, const int32_t *d_neighbours, int n_candidates, const int32_t *bad_maps, int n_bad,
        int max_list, int32_t *d_counts, orbhip_kfdb_entry *d_list, orbhip_kfdb_candidate *d_scored, int32_t *d_loop, int32_t *d_merge,
        int32_t *d_ncand, int32_t *d_reloc, int32_t *d_nreloc);
orbhip_ctx *orbhip_kfdb_ctx_internal(orbhip_kfdb *db);
int orbhip_kfdb_max_words_internal(orbhip_kfdb *db);

// preint_kernels.hip: the argument rules of orbhip_preintegrate_device / _host (one statement for both: before the offsets are at hand,
// and on the offsets in HOST memory), and the launches with checked arguments
int orbhip_preint_check_args_internal(const orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const void *meas_off, const void *record,
        const void *cov, const void *avg, const void *info, const void *info_g, const void *info_a);
int orbhip_preint_check_offsets_internal(const int32_t *off, int chains, const void *meas);
int orbhip_preint_launch_internal(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *d_meas_off, const float *d_meas,
        const uint8_t *d_continue, double *d_record, float *d_cov, float *d_avg, double *d_info, double *d_info_g, double *d_info_a);

// a failed HIP call: its text becomes the last error, the enclosing function returns ORBHIP_E_HIP
#define ORB_HIP_TRY(e) do { if ((e) != hipSuccess) { orbhip_set_last_error_internal(#e); return ORBHIP_E_HIP; } } while (0)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// an arena cut into typed blocks, each rounded up to 256 bytes; off is the size so far.  base == nullptr: only the size is wanted
struct Carve {
    char *base; size_t off = 0;
    template <class T> T *take(size_t count) { T *p = base ? reinterpret_cast<T *>(base + off) : nullptr; off += align256(count * sizeof(T)); return p; }
};
