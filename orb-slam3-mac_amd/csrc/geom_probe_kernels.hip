// geom_probe_kernels.hip -- every shared SO(3) / Sim(3) / SE(3) / camera primitive run ALONE on the device, for the tests
// (tests/test_gpu_geom_probe.py): geom3.h, so3_f64.h, sim3_group.h, se3_oplus / se3_mul of ba_edges.h, ba_camera.h, cam_project_f32.h, svd4.h.
// One lane per item, one kernel per op (a primitive's registers or scratch do not touch another's): the lane copies its input row to
// locals, calls the primitive, writes its output row; nothing else is computed on the device.
//
// Contraction: this file sets NO pragma of its own, so the library's -ffp-contract=off holds for ba_camera.h, cam_project_f32.h and svd4.h
// as in their real includers (which include them before their own pragma, or have none); every other header opens each body with its own.
// One double interface: the float primitives receive doubles that hold float-exact values and cast here, both directions exact.
//
// What this proves is the TEXT of each primitive (formula, branch, threshold, pivot order); it does not prove the instruction schedule a
// solver kernel ends up with after inlining (DESIGN "geom probe").  Debug only; not a product path.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "so3_f64.h"         // geom3.h
#include "sim3_group.h"
#include "ba_edges.h"        // se3_oplus, se3_mul; ba_camera.h
#include "cam_project_f32.h"
#include "svd4.h"
#include <cstring>

namespace {

#define GP_MAX_ITEMS 65536
#define GP_BLOCK 64

// k_gp_<name>: a[IW] in, o[OW] out
#define GP_KERNEL(NAME, IW, OW, ...)                                                                   \
    __global__ __launch_bounds__(GP_BLOCK) void k_gp_##NAME(const double *in, int n, double *out)      \
    {                                                                                                  \
        const int it = blockIdx.x * GP_BLOCK + threadIdx.x;                                            \
        if (it >= n) return;                                                                           \
        double a[IW], o[OW];                                                                           \
        _Pragma("unroll") for (int k = 0; k < IW; k++) a[k] = in[(size_t)it * IW + k];                 \
        { __VA_ARGS__ }                                                                                \
        _Pragma("unroll") for (int k = 0; k < OW; k++) out[(size_t)it * OW + k] = o[k];                \
    }

GP_KERNEL(quat_to_R, 4, 9, quat_to_R(a, o);)
GP_KERNEL(R_to_quat, 9, 4, R_to_quat(a, o);)
GP_KERNEL(quat_rot, 7, 3, quat_rot(a, a + 4, o);)
GP_KERNEL(quat_mul, 8, 4, quat_mul(a, a + 4, o);)
GP_KERNEL(quat_norm_rot, 4, 4, for (int k = 0; k < 4; k++) o[k] = a[k]; quat_norm_rot(o);)
GP_KERNEL(huber, 3, 2, huber(a[0], a[1], a[2], &o[0], &o[1]);)
GP_KERNEL(se3_oplus, 13, 7, se3_oplus(a, a + 6, o);)
GP_KERNEL(se3_mul, 14, 7, se3_mul(a, a + 7, o);)
GP_KERNEL(so3_exp, 3, 9, so3_exp(a, o, 1e-5, true);)             // G2oTypes.cc ExpSO3
GP_KERNEL(so3_exp_imu, 3, 9, so3_exp(a, o, 1e-4, false);)        // ImuTypes.cc, the preintegration's
GP_KERNEL(so3_log, 9, 3, so3_log(a, o);)
GP_KERNEL(so3_right_jac, 3, 9, so3_right_jac(a, o);)
GP_KERNEL(so3_inv_right_jac, 3, 9, so3_inv_right_jac(a, o);)
GP_KERNEL(so3_normalize, 9, 9, for (int k = 0; k < 9; k++) o[k] = a[k]; so3_normalize(o);)
GP_KERNEL(s3_exp, 7, 8, s3_exp(a, o);)
GP_KERNEL(s3_log, 8, 7, s3_log(a, o);)
GP_KERNEL(s3_mul, 16, 8, s3_mul(a, a + 8, o);)
GP_KERNEL(s3_inverse, 8, 8, s3_inverse(a, o);)
GP_KERNEL(s3_map, 11, 3, s3_map(a, a + 8, o);)
// (fx fy cx cy model k0 k1 k2 k3 | P)
GP_KERNEL(cam_project, 12, 2, cam_project(a[0], a[1], a[2], a[3], (int)a[4], a + 5, a + 9, o);)
GP_KERNEL(cam_project_jac, 12, 6, cam_project_jac(a[0], a[1], (int)a[4], a + 5, a + 9, o);)
// float ops: (p[8] = fx fy cx cy k0 k1 k2 k3 | P) and (p[8] | u v); the camera type is the op's
#define GP_TRI_PROJECT(TYPE)                                                          \
    float p[8], P[3], uv[2];                                                          \
    for (int k = 0; k < 8; k++) p[k] = (float)a[k];                                   \
    for (int k = 0; k < 3; k++) P[k] = (float)a[8 + k];                               \
    tri_project(TYPE, p, P, uv);                                                      \
    o[0] = (double)uv[0]; o[1] = (double)uv[1];
#define GP_TRI_UNPROJECT(TYPE)                                                        \
    float p[8], ray[3];                                                               \
    for (int k = 0; k < 8; k++) p[k] = (float)a[k];                                   \
    tri_unproject(TYPE, p, (float)a[8], (float)a[9], ray);                            \
    for (int k = 0; k < 3; k++) o[k] = (double)ray[k];
GP_KERNEL(tri_project_pinhole, 11, 2, GP_TRI_PROJECT(0))
GP_KERNEL(tri_project_kb8, 11, 2, GP_TRI_PROJECT(1))
GP_KERNEL(tri_unproject_pinhole, 10, 3, GP_TRI_UNPROJECT(0))
GP_KERNEL(tri_unproject_kb8, 10, 3, GP_TRI_UNPROJECT(1))
// in[4 * i + k] = At[i][k], At[i] = column i of A
GP_KERNEL(tri_svd4_null, 16, 4,
          float At[4][4]; float v[4];
          for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) At[i][k] = (float)a[4 * i + k];
          tri_svd4_null(At, v);
          for (int k = 0; k < 4; k++) o[k] = (double)v[k];)

struct GpOp { void (*kernel)(const double *, int, double *); int in_width, out_width; };
#define GP_OP(NAME, IW, OW) {k_gp_##NAME, IW, OW}
// the ids are orbhip.h's ORBHIP_GEOM_* in order
const GpOp GP_OPS[ORBHIP_GEOM_N_OPS] = {
    GP_OP(quat_to_R, 4, 9), GP_OP(R_to_quat, 9, 4), GP_OP(quat_rot, 7, 3), GP_OP(quat_mul, 8, 4), GP_OP(quat_norm_rot, 4, 4), GP_OP(huber, 3, 2),
    GP_OP(se3_oplus, 13, 7), GP_OP(se3_mul, 14, 7), GP_OP(so3_exp, 3, 9), GP_OP(so3_exp_imu, 3, 9), GP_OP(so3_log, 9, 3),
    GP_OP(so3_right_jac, 3, 9), GP_OP(so3_inv_right_jac, 3, 9), GP_OP(so3_normalize, 9, 9), GP_OP(s3_exp, 7, 8), GP_OP(s3_log, 8, 7),
    GP_OP(s3_mul, 16, 8), GP_OP(s3_inverse, 8, 8), GP_OP(s3_map, 11, 3), GP_OP(cam_project, 12, 2), GP_OP(cam_project_jac, 12, 6),
    GP_OP(tri_project_pinhole, 11, 2), GP_OP(tri_project_kb8, 11, 2), GP_OP(tri_unproject_pinhole, 10, 3), GP_OP(tri_unproject_kb8, 10, 3),
    GP_OP(tri_svd4_null, 16, 4),
};

int gp_fail(int code, const char *msg) { orbhip_set_last_error_internal(msg); return code; }

}  // namespace

extern "C" int orbhip_debug_geom_probe_host(orbhip_ctx *ctx, int op, const double *in, int n, int in_width, double *out, int out_width)
{
#define GP_FN "orbhip_debug_geom_probe_host: "
    if (!ctx) return gp_fail(ORBHIP_E_BADARG, GP_FN "ctx is NULL");
    if (op < 0 || op >= ORBHIP_GEOM_N_OPS) return gp_fail(ORBHIP_E_BADARG, GP_FN "unknown op");
    const GpOp &O = GP_OPS[op];
    if (in_width != O.in_width || out_width != O.out_width) return gp_fail(ORBHIP_E_BADARG, GP_FN "in_width / out_width are not the op's");
    if (n < 0) return gp_fail(ORBHIP_E_BADARG, GP_FN "n < 0");
    if (n > GP_MAX_ITEMS) return gp_fail(ORBHIP_E_CAPACITY, GP_FN "more than 65536 items");
    if (n == 0) return ORBHIP_OK;
    if (!in || !out) return gp_fail(ORBHIP_E_BADARG, GP_FN "in / out is NULL");
    const size_t nin = (size_t)n * O.in_width, nout = (size_t)n * O.out_width;
    double *h = (double *)orbhip_ctx_pinned_internal(ctx, sizeof(double) * (nin + nout));
    if (!h) return ORBHIP_E_HIP;
    double *d = (double *)orbhip_ctx_work_internal(ctx, sizeof(double) * (nin + nout));
    if (!d) return ORBHIP_E_HIP;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    memcpy(h, in, sizeof(double) * nin);
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    ORB_HIP_TRY(hipMemcpyAsync(d, h, sizeof(double) * nin, hipMemcpyHostToDevice, s));
    O.kernel<<<(n + GP_BLOCK - 1) / GP_BLOCK, GP_BLOCK, 0, s>>>(d, n, d + nin);
    if (hipGetLastError() != hipSuccess) return gp_fail(ORBHIP_E_HIP, GP_FN "the kernel launch failed");
    ORB_HIP_TRY(hipMemcpyAsync(h + nin, d + nin, sizeof(double) * nout, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    memcpy(out, h + nin, sizeof(double) * nout);          // rows past n are the caller's
    return ORBHIP_OK;
#undef GP_FN
}
