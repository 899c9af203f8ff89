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

// a failed HIP call: its text becomes the last error, the enclosing function returns ORBHIP_E_HIP
#define ORB_HIP_TRY(e) do { if ((e) != hipSuccess) { orbhip_set_last_error_internal(#e); return ORBHIP_E_HIP; } } while (0)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
