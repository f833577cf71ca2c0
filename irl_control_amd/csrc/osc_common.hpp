// Shared device-side pieces of the OSC kernels (gfx950 / CDNA4 only).
//
// Everything here restates arithmetic of /root/reference/irl_control/osc.py; the line references
// in the comments are to that file unless another file is named.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/irlosc.h"

namespace irlosc {

// Copy of a plain struct that may live in the constant address space (train tables are read through it so that
// the loads are scalar): C++ will not bind an implicit copy constructor across address spaces.
template <typename T>
__device__ __forceinline__ T pod_copy(const T& src) { return src; }
template <typename T>
__device__ __forceinline__ T pod_copy(const __attribute__((address_space(4))) T& src) {
    static_assert(sizeof(T) % 4 == 0, "word-wise copy");
    T dst;
    const __attribute__((address_space(4))) uint32_t* w = (const __attribute__((address_space(4))) uint32_t*)&src;
    uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) d[i] = w[i];
    return dst;
}

// Per-target-device metadata, broadcast to every instance (lives in kernarg/SGPR space).
struct DevMeta {
    int32_t row0;         // first row of this device's block in the stacked J / task vector
    int32_t rows;         // r_d
    uint32_t dofmask;     // bits 0..5 = ctrlr_dof (device.py:36)
    uint32_t calc;        // bit0: xyz error computed (osc.py:108), bit1: abg error computed (osc.py:113)
    uint32_t joint_mask;  // bit j: position j belongs to device.joint_ids_all (osc.py:174)
    int32_t jidx0;        // first dx row used by the target-velocity branch (robot.py:50-55)
};

template <typename T>
struct KParams {
    const T* M;
    const T* J;
    const T* dq;
    const T* bias;
    const T* ee;      // [B][ndev][7]
    const T* tgt;     // [B][ndev][7]
    const T* tvel;    // [B][ndev][6] or nullptr
    const T* wrench;  // [B][ndev][6] or nullptr
    T* u;             // [B][n]
    uint32_t* flags;  // [B]
    const T* gains;   // [nb][ndev][12]
    const T* null_kv; // [nb]
    const int32_t* index;        // optional worklist of instance ids (nullptr = identity)
    const int32_t* index_count;  // device-side length of the worklist (grid-strided) when index != nullptr
    int32_t b0;                  // first instance handled by block 0 when index == nullptr
    unsigned long long* dbg;     // phase-timing buffer (IRLOSC_PHASE_TIMING=1 debug runs), else nullptr
    int32_t gains_per_instance;
    int32_t B, n, k, ndev;
    uint32_t cfgflags;
    int32_t padded;              // host-side launch choice (irlosc_create: IRLOSC_CLASS_ROW16_PADDED): the KMAX-padded row16 variant; kernels ignore it
    DevMeta dev[IRLOSC_MAX_DEV];
};

// ---- scalar math wrappers -----------------------------------------------------------------------
__device__ __forceinline__ float t_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double t_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float t_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double t_abs(double x) { return fabs(x); }
__device__ __forceinline__ float t_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double t_atan2(double y, double x) { return atan2(y, x); }
template <typename T> struct Eps;
template <> struct Eps<float> { static constexpr float v = 1.1920929e-7f; };
template <> struct Eps<double> { static constexpr double v = 2.220446049250313e-16; };

__device__ __forceinline__ bool t_finite(float x) { return fabsf(x) <= 3.4028235e38f; }
__device__ __forceinline__ bool t_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// ---- compile-time loops: f(std::integral_constant<int, i>{}) for i = B_ .. E_ - 1, resp. E_ - 1 down to B_ ------------------------
template <int B_, int E_, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B_ < E_) {
        f(std::integral_constant<int, B_>{});
        static_for<B_ + 1, E_>(f);
    }
}
template <int B_, int E_, typename F>
__device__ __forceinline__ void static_for_down(F&& f) {
    if constexpr (B_ < E_) {
        f(std::integral_constant<int, E_ - 1>{});
        static_for_down<B_, E_ - 1>(f);
    }
}

// 1/sqrt(d) and 1/d to fp64 accuracy from the 2^-24 hardware seeds (one cubic / quadratic correction; measured
// max relative error 2.6e-16 and 0 against 1/sqrt and 1/ of the host, tools/probe/dpp64.hip)
__device__ __forceinline__ double rsq_refined(double d) {
    const double q = __builtin_amdgcn_rsq(d);
    const double e = fma(-(d * q), q, 1.0);
    return fma(q * e, fma(0.375, e, 0.5), q);
}
__device__ __forceinline__ double rcp_refined(double d) {
    const double r = __builtin_amdgcn_rcp(d);
    const double e = fma(-d, r, 1.0);
    return fma(r * e, 1.0 + e, r);
}
__device__ __forceinline__ double sqrt_fast(double x) { return x > 0.0 ? x * rsq_refined(x) : 0.0; }

// ---- task-space error of one device (calc_error, osc.py:101-118) ----------------------------------
// ee/tg: x y z qw qx qy qz.  The quaternion part restates the transforms3d calls made there:
// q_d = normalized_vector(tgt_quat); q_r = qmult(q_d, qconjugate(q_ee)); e[3:] = quat2euler(qconjugate(q_r))
// with quat2euler(axes='sxyz') = mat2euler(quat2mat(q)).
template <typename T>
__device__ __forceinline__ void task_error6(const T* __restrict__ ee, const T* __restrict__ tg,
                                            bool cx, bool ca, T e[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = T(0);
    if (cx) {
        e[0] = ee[0] - tg[0];
        e[1] = ee[1] - tg[1];
        e[2] = ee[2] - tg[2];
    }
    if (ca) {
        T tw = tg[3], tx = tg[4], ty = tg[5], tz = tg[6];
        T nrm = t_sqrt(tw * tw + tx * tx + ty * ty + tz * tz);
        T w1 = tw / nrm, x1 = tx / nrm, y1 = ty / nrm, z1 = tz / nrm;  // q_d
        T w2 = ee[3], x2 = -ee[4], y2 = -ee[5], z2 = -ee[6];            // conj(q_ee)
        // Hamilton product q_r = q_d * conj(q_ee)
        T rw = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
        T rx = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
        T ry = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2;
        T rz = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2;
        // q = conj(q_r)
        T w = rw, x = -rx, y = -ry, z = -rz;
        T Nq = w * w + x * x + y * y + z * z;
        T r00 = T(1), r10 = T(0), r20 = T(0), r21 = T(0), r22 = T(1), r11 = T(1), r12 = T(0);
        if (!(Nq < T(2.220446049250313e-16))) {
            T s = T(2) / Nq;
            T X = x * s, Y = y * s, Z = z * s;
            T wX = w * X, wY = w * Y, wZ = w * Z;
            T xX = x * X, xY = x * Y, xZ = x * Z;
            T yY = y * Y, yZ = y * Z, zZ = z * Z;
            r00 = T(1) - (yY + zZ);
            r10 = xY + wZ;
            r20 = xZ - wY;
            r21 = yZ + wX;
            r22 = T(1) - (xX + yY);
            r11 = T(1) - (xX + zZ);
            r12 = yZ - wX;
        }
        T cy = t_sqrt(r00 * r00 + r10 * r10);
        if (cy > T(4.0 * 2.220446049250313e-16)) {
            e[3] = t_atan2(r21, r22);
            e[4] = t_atan2(-r20, cy);
            e[5] = t_atan2(r10, r00);
        } else {
            e[3] = t_atan2(-r12, r11);
            e[4] = t_atan2(-r20, cy);
            e[5] = T(0);
        }
    }
}

// Gains record: kp kv ko k0 k1 k2 d0 d1 d2 max_vel0 max_vel1 has_max_vel
// Velocity limiting + gains + stiffness (osc.py:70-99 and 160-168).  e is updated in place.
template <typename T>
__device__ __forceinline__ void apply_gains6(const T* __restrict__ g, T e[6]) {
    const T kp = g[0], kv = g[1], ko = g[2];
    if (g[11] != T(0)) {
        T sx = T(1), sa = T(1);
        T nx = t_sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        T satx = g[9] / kp * kv;
        if (nx > satx) sx = sx * (satx / nx);
        T na = t_sqrt(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
        T sata = g[10] / ko * kv;
        if (na > sata) sa = sa * (sata / na);
        T lp = kp / kv, lo = ko / kv;  // lamb (osc.py:39)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            e[i] = kv * sx * lp * e[i];
            e[3 + i] = kv * sa * lo * e[3 + i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) e[i] *= g[3 + i];  // stiffness k; abg entries are 1
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            e[i] *= kp * g[3 + i];
            e[3 + i] *= ko;
        }
    }
}

// Wave-wide sum over 64 lanes (result in every lane).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        T o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The TARGET TILE of the kernels that write a slot's targets inside a rollout (osc_waypoint.hpp, osc_action.hpp, osc_teleop.hpp: one block per walk
// wave, one lane per robot).  The target record tgt[B][ndev][7] is row-major in the record type T, a lane's words 7 ndev apart, so the
// wave's tile -- the rows of its nvalid robots, tg = tgt + b0 * row, row = ndev * 7 -- goes through LDS.  The contract: the tile stays
// in the record type and is stored whole, so a word no lane rewrote goes back bit for bit; it is stored only by a wave in which a lane
// moved a target; idle lanes of a ragged last wave (nvalid < 64) neither load nor store: only the wave's robots' words are touched.
template <typename T>
__device__ __forceinline__ void tgt_tile_load(T* s_t, const T* tg, int nvalid, int row) {
    for (int t = 0; t < row; ++t) {
        const int i = t * 64 + (int)threadIdx.x;
        if (i < nvalid * row) s_t[i] = tg[i];
    }
    __syncthreads();
}
template <typename T>
__device__ __forceinline__ void tgt_tile_store(T* tg, const T* s_t, int nvalid, int row, bool moved) {
    if (!__any(moved)) return;                      // (one wave per block: uniform over the block)
    __syncthreads();
    for (int t = 0; t < row; ++t) {
        const int i = t * 64 + (int)threadIdx.x;
        if (i < nvalid * row) tg[i] = s_t[i];
    }
}

// Quaternion helpers of the rollout's float64 program kernels (osc_teleop.hpp, osc_object.hpp, osc_action.hpp): every product and sum
// rounded on its own and in the order written, so that the host can repeat the bits with plain NumPy expressions.
//   r = a (x) b, the Hamilton product (w x y z), terms left to right; no normalisation, no sign change
__device__ __forceinline__ void quat_mul_rn(const double a[4], const double b[4], double r[4]) {
    r[0] = __dsub_rn(__dsub_rn(__dsub_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2])), __dmul_rn(a[3], b[3]));
    r[1] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0])), __dmul_rn(a[2], b[3])), __dmul_rn(a[3], b[2]));
    r[2] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], b[2]), __dmul_rn(a[2], b[0])), __dmul_rn(a[3], b[1])), __dmul_rn(a[1], b[3]));
    r[3] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], b[3]), __dmul_rn(a[3], b[0])), __dmul_rn(a[1], b[2])), __dmul_rn(a[2], b[1]));
}
//   R(q): transforms.quat2mat without its Nq < eps branch (the callers' quaternions are of unit length to rounding); the one division,
//   2 / Nq, is correctly rounded like the products
__device__ __forceinline__ void quat2mat_rn(const double q[4], double R[3][3]) {
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double Nq = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(qw, qw), __dmul_rn(qx, qx)), __dmul_rn(qy, qy)), __dmul_rn(qz, qz));
    const double s = __ddiv_rn(2.0, Nq);
    const double X = __dmul_rn(qx, s), Y = __dmul_rn(qy, s), Z = __dmul_rn(qz, s);
    const double wX = __dmul_rn(qw, X), wY = __dmul_rn(qw, Y), wZ = __dmul_rn(qw, Z);
    const double xX = __dmul_rn(qx, X), xY = __dmul_rn(qx, Y), xZ = __dmul_rn(qx, Z);
    const double yY = __dmul_rn(qy, Y), yZ = __dmul_rn(qy, Z), zZ = __dmul_rn(qz, Z);
    R[0][0] = __dsub_rn(1.0, __dadd_rn(yY, zZ)); R[0][1] = __dsub_rn(xY, wZ); R[0][2] = __dadd_rn(xZ, wY);
    R[1][0] = __dadd_rn(xY, wZ); R[1][1] = __dsub_rn(1.0, __dadd_rn(xX, zZ)); R[1][2] = __dsub_rn(yZ, wX);
    R[2][0] = __dsub_rn(xZ, wY); R[2][1] = __dadd_rn(yZ, wX); R[2][2] = __dsub_rn(1.0, __dadd_rn(xX, yY));
}
//   R v and R^T v, each row's three products summed left to right
__device__ __forceinline__ void mat_vec_rn(const double R[3][3], const double v[3], double r[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = __dadd_rn(__dadd_rn(__dmul_rn(R[c][0], v[0]), __dmul_rn(R[c][1], v[1])), __dmul_rn(R[c][2], v[2]));
}
__device__ __forceinline__ void mat_t_vec_rn(const double R[3][3], const double v[3], double r[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = __dadd_rn(__dadd_rn(__dmul_rn(R[0][c], v[0]), __dmul_rn(R[1][c], v[1])), __dmul_rn(R[2][c], v[2]));
}

// zero pattern asked of dense records (osc_structure_kernel): bit c of mrow[j]: M[j][c] may be non-zero; bit c of jcols: column c of J
struct StructureMasks { uint32_t mrow[32]; uint32_t jcols; };

}  // namespace irlosc
