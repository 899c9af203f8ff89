// imu_layout.h -- where the fields of an inertial keyframe state (ORBHIP_IBA_KF doubles) and of a preintegration record
// (ORBHIP_IBA_PREINT doubles) sit, as include/orbhip.h documents them, and the gravity constant: one statement for the inertial BA
// (iba_edges.h, iba_kernels.hip), the inertial pose-only optimisation (pose_inertial_kernels.hip) and the inertial initialisation
// (inertial_opt_kernels.hip).  Nothing from HIP is included.
#pragma once

// keyframe state: Rwb[9] (row-major), twb[3], velocity[3], gyro bias[3], accelerometer bias[3]
enum { K_R = 0, K_T = 9, K_V = 12, K_BG = 15, K_BA = 18 };
// preintegration: dT, dR[9], dV[3], dP[3], the bias Jacobians JRg / JVg / JVa / JPg / JPa [9] each, the bias it was integrated at (gyro, acc)
enum { P_DT = 0, P_DR = 1, P_DV = 10, P_DP = 13, P_JRG = 16, P_JVG = 25, P_JVA = 34, P_JPG = 43, P_JPA = 52, P_BG = 61, P_BA = 64 };
static_assert(K_BA + 3 == 21 && P_BA + 3 == 67, "the layouts fill ORBHIP_IBA_KF = 21 and ORBHIP_IBA_PREINT = 67 doubles");

#define IMU_GRAVITY ((double)9.81f)     // IMU::GRAVITY_VALUE (include/ImuTypes.h) is a float constant
