// The POLICY of a rollout (irlosc_set_policy): per tick and robot a small ReLU network maps the tick's observation to the space-mouse
// reading of the tick, and the stream's own body (osc_teleop.hpp::teleop_follow) integrates it into the plate pose and writes the
// followers' targets -- so that the OSC step of the SAME tick aims at them without the host in between.  It runs where the stream kernel
// runs: behind the walk, the feed's wrench with every SENSE launch and the object kernel, in front of the first OSC kernel.
//
// One block per walk wave (its 64 robots), like the stream kernel, but of FOUR waves: the activations of 64 robots fill most of a CU's LDS
// at the upper end, so one block is resident per CU, and its four waves put the CU's four SIMDs to work on the layers' output tiles.  Three phases:
//   GATHER   the wave's observation tile x[k][robot] (float, LDS, POLICY_XS words per row) from where the operands lie: qt and the
//            exchange block [entry][64] (one coalesced line per word), the target tile (osc_common.hpp: its contract -- loaded here,
//            read for IRLOSC_OBS_TARGETS, stored at the end), the wrench rows, the SoA plate and object state.  Idle lanes of a ragged
//            wave hold zeros.  With keep_obs the tile is stored row-major, coalesced.
//   LAYERS   on v_mfma_f32_16x16x4_f32: outputs on the rows of a 16 x 16 tile (A = the weights), robots on its columns (B = x), four
//            robot tiles per wave -- four independent accumulators, which is what the instruction's 40-cycle dependent latency against
//            its 32-cycle issue asks for.  An accumulator starts as the bias and takes the k-steps in ascending order, so that every
//            output is the chain acc = fmaf(W[j][i], x[i], acc), i ascending (include/irlosc.h: the arithmetic).  A layer's result goes
//            back to LDS in [output][robot] order -- the next layer's k is this layer's output index, ascending again; feeding the
//            accumulator registers straight back would permute k.  Two LDS buffers alternate.  A operands come from the setter's packed
//            copy of the weights: fragment (layer, output tile, k-step) is 64 consecutive floats, lane l holding W[16 ot + (l & 15)][4 ks
//            + (l >> 4)] -- one coalesced 256-byte load that hits in L2 (the largest network is 295 KB: not LDS material).  B operands:
//            lane l reads x[4 ks + (l >> 4)][16 rt + (l & 15)]; POLICY_XS = 80 puts the four rows of a k-step on disjoint banks.
//   FOLLOW   wave 0, lane = robot again: its n_out outputs from LDS, the finiteness verdict, clamp, teleop_follow, grip; the tile is stored.
// A robot whose observation or output holds a non-finite word is skipped in FOLLOW (pose, targets, out, grip stay) and gets
// IRLOSC_FLAG_NONFINITE in flags_any: a robot is a COLUMN of every product, so its words never meet another robot's.
// Cost per wave: sum over layers of 4 ceil(out / 16) ceil(in / 4) MFMAs at 32 cycles: the floor profiles/policy_rates.md measures against.
//
// The GAUSSIAN HEAD (irlosc_set_policy_noise; the NOISE = true form of the kernel, which only a slot with a head launches): the network's
// output is the MEAN, the action that steers the plate is act[c] = mean[c] + std[c] eps[c], and the robot's log-probability of it is kept.
//   DRAW     in front of LAYERS, all four waves, lane = robot: eps[c] = z[c & 3] of Philox block (robot, draws, c >> 2, stream 1)
//            (osc_rng.hpp: normal4), so two blocks of two Box-Muller pairs cover 6 or 7 outputs -- four equal pieces, one per wave: wave wv
//            computes block wv >> 1 and of it the pair wv & 1, and leaves its two normals in the eps region [8][64] (double) of LDS behind
//            the activation buffers.  The draw reads nothing of the network, so its fp64 VALU work is issued where the MFMA pipe is about to
//            be busy; the barriers of LAYERS stand between its stores and FOLLOW's loads.
//   FOLLOW   act, logp = -s / 2 - C with s the sum of eps[c]^2 over the noisy outputs (include/irlosc.h: the arithmetic), the verdict on
//            observation, mean AND act, and everything behind the network on act where the plain form has out.  draws[robot] advances by
//            one on every tick that runs the robot, finite or not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"
#include "osc_rng.hpp"
#include "osc_teleop.hpp"

namespace irlosc {

constexpr int POLICY_WAVES = 4;    // waves of a block: they share the block's 64 robots and split every layer's output tiles (one per SIMD)
constexpr int POLICY_KC = 8;       // k-steps whose A fragments are loaded ahead of their MFMAs
constexpr int POLICY_XS = 80;      // floats between two rows of an LDS activation buffer (64 robots + 16: rows k .. k + 3 on disjoint banks)

// The packed network: per layer its k-steps (padded inputs / 4), output tiles (padded outputs / 16) and where its fragments
// [ot][ks][64] and its padded bias [16 ot] start in the packed array, in floats
struct PolicyNet {
    int32_t L, n_in, n_out;
    int32_t ksteps[IRLOSC_POLICY_MAX_LAYERS], otiles[IRLOSC_POLICY_MAX_LAYERS];
    int32_t woff[IRLOSC_POLICY_MAX_LAYERS], boff[IRLOSC_POLICY_MAX_LAYERS];
    int32_t rows[2];               // rows of the two LDS buffers: layer l reads buffer l & 1 and writes the other
};

// The policy's per-robot state besides the plate (PlateState): out [n_out][stride], grip [stride]; with a Gaussian head (act != nullptr)
// act [n_out][stride], logp [stride] and draws [stride], the ticks that ran the robot since the head's setter (plus its draw0; mod 2^32)
struct PolicyState { float* out; double* grip; float* act; double* logp; uint32_t* draws; };
// One robot's fresh outputs (so: its column): what the fills of irlosc_set_policy and irlosc_set_policy_noise leave, written by a reset of
// episodes.  draws stays: it counts on across resets, so that every episode explores afresh.
__device__ __forceinline__ void policy_fresh(PolicyState st, int n_out, int stride, size_t so) {
    for (int c = 0; c < n_out; ++c) st.out[(size_t)c * stride + so] = 0.0f;
    st.grip[so] = 0.0;
    if (st.act) {
        for (int c = 0; c < n_out; ++c) st.act[(size_t)c * stride + so] = 0.0f;
        st.logp[so] = 0.0;
    }
}

struct PolicyArgs {
    TeleopArgs t;                  // tgt, the plate, inc, the rig, B, ndev, stride: what teleop_follow reads (the stream's other fields: 0)
    PolicyNet net;
    const float* w;                // the packed weights
    const double* qt;              // [walk wave][2 n][64]: entry 2 j = q_j, 2 j + 1 = qd_j
    const double* xside;           // the tick's exchange block [walk wave][n_entries][64]
    const void* wrench;            // [B][ndev][6], record type: the feed's wrench of the tick, or nullptr (no feed: zeros)
    const double* obj_pose;        // [IRLOSC_MAX_OBJECTS 7][stride]
    PolicyState st;
    float* obs;                    // [B][n_in] row-major, or nullptr (keep_obs == 0)
    uint32_t* flags_any;           // [B] of the rollout call
    double grip_close, grip_open;
    float clip;
    uint32_t obs_mask;
    int32_t n, n_entries, nobj;
    int32_t ee0[IRLOSC_MAX_DEV];   // exchange entry of each device's EE pose
    // the Gaussian head (read by the NOISE form alone): the key, std[c] (0: output c is deterministic) and C of logp = -s / 2 - C
    uint64_t seed;
    double logp_const;
    float std[8];
};

typedef float policy_f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t POLICY_EPS_BYTES = 8 * 64 * sizeof(double);      // the head's eps region [8][64]: 4 KB behind the activation buffers

// LDS of a launch: the target tile and the block's verdict word (a 16-byte multiple), then the two activation buffers, then (a head) the eps region
template <typename T>
__host__ __device__ inline size_t policy_tile_bytes(int ndev) { return (((size_t)64 * ndev * 7 * sizeof(T) + 15) & ~(size_t)15) + 16; }
template <typename T>
inline size_t policy_lds_bytes(const PolicyNet& n, int ndev, bool noise = false) {
    return policy_tile_bytes<T>(ndev) + (size_t)(n.rows[0] + n.rows[1]) * POLICY_XS * sizeof(float) + (noise ? POLICY_EPS_BYTES : 0);
}

template <typename T, bool NOISE>
__global__ __launch_bounds__(64 * POLICY_WAVES) void osc_policy_kernel(const PolicyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;      // wv: the wave of the block (uniform over a wave)
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.t.B - b0);         // robots of this block
    const bool valid = lane < nvalid;
    const size_t so = (size_t)b0 + lane;
    const int ndev = a.t.ndev, row = ndev * 7, stride = a.t.stride;
    T* s_t = (T*)s_raw;                             // the block's target tile
    float* xb[2];
    xb[0] = (float*)(s_raw + policy_tile_bytes<T>(ndev));
    xb[1] = xb[0] + (size_t)a.net.rows[0] * POLICY_XS;
    int* s_moved = (int*)xb[0] - 4;                 // 1: a robot of the block moved its targets (block-uniform once behind a barrier)
    T* __restrict__ tg = (T*)a.t.tgt + (size_t)b0 * row;
    tgt_tile_load(s_t, tg, nvalid, row);            // (every wave passes over the tile: the words are the same, the barrier is the block's)

    // ---- GATHER: x[k][lane], k ascending in bit order, wave wv the words k = wv, wv + POLICY_WAVES, ... of every channel.  An idle lane loads
    // what the block's first robot loads and keeps a zero: every load is unconditional, so that a channel's loads are in flight together ----
    float* __restrict__ x0 = xb[0] + lane;
    const int lc = valid ? lane : 0;
    const size_t sc = (size_t)b0 + lc;
    auto word = [&](auto v) { return valid ? (float)v : 0.0f; };
    int k = 0;
    if (a.obs_mask & (IRLOSC_OBS_QPOS | IRLOSC_OBS_QVEL)) {
        const double* __restrict__ col = a.qt + (size_t)blockIdx.x * (2 * a.n * 64) + lc;
        for (int h = 0; h < 2; ++h) {
            if (!(a.obs_mask & (h ? IRLOSC_OBS_QVEL : IRLOSC_OBS_QPOS))) continue;
            for (int j = wv; j < a.n; j += POLICY_WAVES) x0[(k + j) * POLICY_XS] = word(col[(size_t)(2 * j + h) * 64]);
            k += a.n;
        }
    }
    if (a.obs_mask & IRLOSC_OBS_EE_POSE) {
        const double* __restrict__ col = a.xside + (size_t)blockIdx.x * a.n_entries * 64 + lc;
        for (int i = wv; i < row; i += POLICY_WAVES) x0[(k + i) * POLICY_XS] = word(col[(size_t)(a.ee0[i / 7] + i % 7) * 64]);
        k += row;
    }
    if (a.obs_mask & IRLOSC_OBS_TARGETS) {
        for (int i = wv; i < row; i += POLICY_WAVES) x0[(k + i) * POLICY_XS] = word(s_t[lc * row + i]);
        k += row;
    }
    if (a.obs_mask & IRLOSC_OBS_WRENCH) {
        const int w = ndev * 6;
        const T* __restrict__ wr = (const T*)a.wrench + sc * w;
        if (a.wrench) for (int i = wv; i < w; i += POLICY_WAVES) x0[(k + i) * POLICY_XS] = word(wr[i]);
        else for (int i = wv; i < w; i += POLICY_WAVES) x0[(k + i) * POLICY_XS] = 0.0f;
        k += w;
    }
    if (a.obs_mask & IRLOSC_OBS_PLATE) {
        for (int c = wv; c < 6; c += POLICY_WAVES) x0[(k + c) * POLICY_XS] = word(a.t.st.pose[(size_t)c * stride + sc]);
        k += 6;
    }
    if (a.obs_mask & IRLOSC_OBS_OBJECT_POSE) {
        const int w = a.nobj * 7;
        for (int i = wv; i < w; i += POLICY_WAVES) x0[(k + i) * POLICY_XS] = word(a.obj_pose[(size_t)i * stride + sc]);
        k += w;
    }
    for (k += wv; k < 4 * a.net.ksteps[0]; k += POLICY_WAVES) x0[k * POLICY_XS] = 0.0f;      // the padding of layer 0's inner dimension
    if (threadIdx.x == 0) *s_moved = 0;
    __syncthreads();
    bool finite = true;                             // wave 0, lane = robot: the verdict on its column
    if (wv == 0)
        for (int i = 0; i < a.net.n_in; ++i) finite = finite & (fabsf(x0[i * POLICY_XS]) <= 3.402823466e38f);      // (false for a NaN)
    if (a.obs) {                                    // keep_obs: the tile as [robot][n_in], coalesced
        const int w = a.net.n_in;
        float* __restrict__ o = a.obs + (size_t)b0 * w;
        for (int idx = threadIdx.x; idx < nvalid * w; idx += 64 * POLICY_WAVES) o[idx] = xb[0][(idx % w) * POLICY_XS + idx / w];
    }

    // ---- DRAW (a head): wave wv the pair wv & 1 of block wv >> 1, lane = robot; an idle lane draws what the block's first robot draws ----
    double* s_eps = (double*)(xb[1] + (size_t)a.net.rows[1] * POLICY_XS);      // [8][64] (16-byte aligned: every piece in front is)
    uint32_t drawn = 0;                             // the robot's count of draws at the start of the tick
    if constexpr (NOISE) {
        drawn = a.st.draws[sc];
        const uint32_t ctr[4] = {(uint32_t)sc, drawn, (uint32_t)(wv >> 1), 1u}, key[2] = {(uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
        uint32_t w[4];
        philox4x32_10(ctr, key, w);
        double zc, zs;
        normal_pair((wv & 1) ? w[2] : w[0], (wv & 1) ? w[3] : w[1], &zc, &zs);
        s_eps[(2 * wv) * 64 + lane] = zc;           // (rows 4 (wv >> 1) + 2 (wv & 1) and the next: eps[c] = row c)
        s_eps[(2 * wv + 1) * 64 + lane] = zs;
    }

    // ---- LAYERS: wave wv the output tiles wv, wv + POLICY_WAVES, ... of every layer ----
    const int lr = lane & 15, lq = lane >> 4;
    for (int l = 0; l < a.net.L; ++l) {
        const float* __restrict__ xin = xb[l & 1] + lq * POLICY_XS + lr;
        float* __restrict__ xout = xb[(l & 1) ^ 1] + (4 * lq) * POLICY_XS + lr;
        const int ksteps = a.net.ksteps[l];
        const bool hidden = l + 1 < a.net.L;
        for (int ot = wv; ot < a.net.otiles[l]; ot += POLICY_WAVES) {
            const float* __restrict__ wf = a.w + a.net.woff[l] + (size_t)ot * ksteps * 64 + lane;
            const policy_f32x4 bias = *(const policy_f32x4*)(a.w + a.net.boff[l] + ot * 16 + 4 * lq);
            policy_f32x4 acc[4] = {bias, bias, bias, bias};
            // k-steps in chunks of POLICY_KC: a chunk's A fragments are in registers before its MFMAs start, the next chunk's loads are in
            // flight while they run (an L2 hit is several MFMAs long)
            float an[POLICY_KC];
#pragma unroll
            for (int i = 0; i < POLICY_KC; ++i) an[i] = i < ksteps ? wf[(size_t)i * 64] : 0.0f;
            for (int k0 = 0; k0 < ksteps; k0 += POLICY_KC) {
                float ac[POLICY_KC];
#pragma unroll
                for (int i = 0; i < POLICY_KC; ++i) ac[i] = an[i];
#pragma unroll
                for (int i = 0; i < POLICY_KC; ++i) an[i] = k0 + POLICY_KC + i < ksteps ? wf[(size_t)(k0 + POLICY_KC + i) * 64] : 0.0f;
#pragma unroll
                for (int i = 0; i < POLICY_KC; ++i) {
                    if (k0 + i < ksteps) {              // (uniform; ascending k across the chunk and across chunks)
                        const float* __restrict__ xr = xin + (size_t)(k0 + i) * 4 * POLICY_XS;
#pragma unroll
                        for (int rt = 0; rt < 4; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i], xr[rt * 16], acc[rt], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[rt][r];
                    xout[(size_t)(ot * 16 + r) * POLICY_XS + rt * 16] = hidden ? (v > 0.0f ? v : 0.0f) : v;
                }
        }
        __syncthreads();
    }

    // ---- FOLLOW: wave 0, lane = robot ----
    bool ok = false;
    if (wv == 0) {
        const float* __restrict__ y = xb[a.net.L & 1] + lane;
        float o[7], act[7];                         // the network's output (a head: the mean) and what steers the plate
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            o[c] = c < a.net.n_out ? y[c * POLICY_XS] : 0.0f;
            finite = finite & (fabsf(o[c]) <= 3.402823466e38f);
            act[c] = o[c];
            if constexpr (NOISE) {
                if (c < a.net.n_out && a.std[c] > 0.0f) {      // (uniform; an output with std == 0 keeps the mean's bits)
                    const double eps = s_eps[c * 64 + lane];
                    act[c] = (float)__dadd_rn((double)o[c], __dmul_rn((double)a.std[c], eps));      // (beyond float's range: an infinity)
                    s = __dadd_rn(s, __dmul_rn(eps, eps));
                    finite = finite & (fabsf(act[c]) <= 3.402823466e38f);
                }
            }
        }
        ok = valid && finite;
        if constexpr (NOISE) {
            if (valid) a.st.draws[so] = drawn + 1u; // a tick that ran the robot, finite or not (mod 2^32)
        }
        if (ok) {
            double r[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const float v = act[c];
                r[c] = (double)(a.clip > 0.0f ? (v < -a.clip ? -a.clip : v > a.clip ? a.clip : v) : v);
            }
#pragma unroll
            for (int c = 0; c < 7; ++c)
                if (c < a.net.n_out) a.st.out[(size_t)c * stride + so] = o[c];
            if constexpr (NOISE) {
#pragma unroll
                for (int c = 0; c < 7; ++c)
                    if (c < a.net.n_out) a.st.act[(size_t)c * stride + so] = act[c];
                a.st.logp[so] = __dsub_rn(__dmul_rn(-0.5, s), a.logp_const);
            }
            if (a.net.n_out == 7) a.st.grip[so] = act[6] > 0.0f ? a.grip_close : a.grip_open;
            teleop_follow(a.t, s_t, lane, so, row, r);
        } else if (valid) a.flags_any[so] |= IRLOSC_FLAG_NONFINITE;
        if (__any(ok) && lane == 0) *s_moved = 1;
    }
    __syncthreads();
    tgt_tile_store(tg, s_t, nvalid, row, *s_moved != 0);      // (block-uniform: every wave stores or none; the words are the same)
}

}  // namespace irlosc
