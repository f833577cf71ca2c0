// EXTERNAL PUSHES of a rollout (irlosc_set_pushes): the wrench the reference's admit_test / force_test loops put into xfrc_applied on
// a gripper body during a window of ticks (examples/headless_loops.py::admit_test_loop), and the reaction the F/T sensors read after
// the step that felt it (fakesim.ToyDynamics: s0 - xfrc_applied).  Prescribed by the caller, no contact model.  Two launches of one
// kernel, each only on the ticks the HOST finds a push active for it (the active set is the kernel argument `active`; a tick without
// one launches nothing -- there is no device-side tick state):
//
//   SENSE, between the sensor feed's wrench kernel (osc_ft.hpp) and every kernel that reads the wrench: per device d with a sensed push
//       that was active on the PREVIOUS tick,   wrench[b][d][c] = (T)((double)wrench[b][d][c] - W_d[c])   in the record type T.
//   APPLY, behind the give-up pass and the waypoint cycler, in front of the plant: per device d with an applied push active on THIS
//       tick and every hinge i above its EE body,   bias_i = fma(-J_d[5][i], W_d[5], ... fma(-J_d[0][i], W_d[0], bias_i))   in place
//       on the tick's exchange block, so that the unchanged plant kernel integrates M^-1 (u - bias - damping qvel + sum_d J_d^T W_d).
//       J_d: the six entries per hinge the walk parked behind the EE body's pose (jacp xyz, jacr xyz at the body's frame origin:
//       osc_frontend_lane.hpp, FeTopo::ee_index) -- all six whatever rows the layout controls.  Nothing between the walk and the plant
//       writes those entries or the bias entries, and every OSC kernel of the tick has read the bias by then.
//
// W_d = the wrenches of the active pushes on device d summed in ascending p, the first one taken as it is, every add rounded on its
// own (float64): the host can repeat it (pushes.py).  Devices in ascending d; two devices that name one EE body update its bias one
// after the other.
//
// One lane per robot, one block per walk wave (its 64 robots), like the cycler.  A per-robot table is [walk wave][P 6][64] (every
// operand one coalesced 512-byte line), a shared one [P][6] (scalar loads).  The entry indices of J and the bias are compile-time
// constants of FeTopo<TOPO> per EE-candidate body; the runtime device finds its body by a uniform branch over the candidates, which
// the exchange entry of its pose identifies (PlantArgs::ee0).  Idle lanes of a ragged last wave neither load nor store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_frontend_lane.hpp"

namespace irlosc {

struct PushArgs {
    double* xside;            // apply: the tick's exchange block [walk wave][n_compact][64], bias entries in place
    void* wrench;             // sense: the feed's wrench of the tick [B][ndev][6], record type, in place
    const double* table;      // per_robot: [walk wave][P][6][64], else [P][6]
    int32_t B, ndev, P, per_robot;
    int32_t apply;            // 1: apply mode, 0: sense mode (uniform over the launch)
    uint32_t active;          // bit p: push p is part of this launch's sums (never 0: the host launches nothing then)
    int32_t dev[IRLOSC_MAX_PUSHES];       // target device of push p
    int32_t ee0[IRLOSC_MAX_DEV];          // exchange entry of each device's EE pose: names its EE body
};

// THE CHAIN that takes a wrench W at the frame origin of EE-candidate `body` off the bias, for every hinge i above the body in ascending i:
//     bias_i = fma(-J[5][i], W5, ... fma(-J[0][i], W0, bias_i))
// on the lane's column `col` of the tick's exchange block.  Stated once: the pushes (below) and the carried objects' weight
// (osc_object_load.hpp) both go through it, so a load and a push of the same wrench leave the same bits.
template <class TOPO, int body>
__device__ __forceinline__ void wrench_off_bias(double* __restrict__ col, const double W[6]) {
    using TI = FeTopo<TOPO>;
    constexpr int e0 = TI::ee_index(body);      // (indices through constexpr VARIABLES: evaluated at compile time)
    static_for<0, TOPO::NJ>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (TI::moves(i, body)) {
            constexpr int ej = e0 + 7 + 6 * TI::anc_rank(i, body);
            constexpr int eb = TI::bias_index(i);
            double acc = col[(size_t)eb * 64];
#pragma unroll
            for (int c = 0; c < 6; ++c) acc = fma(-col[(size_t)(ej + c) * 64], W[c], acc);
            col[(size_t)eb * 64] = acc;
        }
    });
}

template <class TOPO, typename T>
__global__ __launch_bounds__(64) void osc_push_kernel(const PushArgs a) {
    using TI = FeTopo<TOPO>;
    constexpr int n_compact = TI::n_compact();
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x * 64 + lane;
    if (b >= a.B) return;                           // (no barrier below)
    const double* __restrict__ tab = a.per_robot ? a.table + (size_t)blockIdx.x * a.P * 6 * 64 + lane : a.table;
    const int cs = a.per_robot ? 64 : 1;
    for (int d = 0; d < a.ndev; ++d) {
        double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool any = false;
        for (int p = 0; p < a.P; ++p) {             // (every condition uniform over the launch: kernel arguments)
            if (!((a.active >> p) & 1u) || a.dev[p] != d) continue;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double w = tab[(size_t)(p * 6 + c) * cs];
                W[c] = any ? __dadd_rn(W[c], w) : w;
            }
            any = true;
        }
        if (!any) continue;
        if (!a.apply) {
            T* w = (T*)a.wrench + ((size_t)b * a.ndev + d) * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c) w[c] = (T)__dsub_rn((double)w[c], W[c]);
            continue;
        }
        double* __restrict__ col = a.xside + (size_t)blockIdx.x * n_compact * 64 + lane;
        const int e0d = a.ee0[d];
        static_for<0, TOPO::NB>([&](auto bc) {
            constexpr int body = decltype(bc)::value;
            if constexpr (TOPO::ee_cand[body] != 0) {
                constexpr int e0 = TI::ee_index(body);
                if (e0d == e0) wrench_off_bias<TOPO, body>(col, W);
            }
        });
    }
}

}  // namespace irlosc
