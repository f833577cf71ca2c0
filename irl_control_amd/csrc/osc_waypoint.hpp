// The WAYPOINT CYCLER of a rollout (irlosc_set_waypoints): per tick, robot and device the index of the reference's caller loops
// (examples/headless_loops.py::gain_test_loop) -- advance when the EE is within the threshold of its target, wrap or finish at the end
// of the list -- and the next waypoint written into the xyz of the slot's target record, so that the next tick's OSC step aims at it
// without the host in between.  It runs between the give-up pass and the plant kernel: every OSC kernel of the tick has read the
// targets by then, and the plant touches neither the EE entries of the exchange block nor the targets.
//
// One lane per robot, one block per walk wave (its 64 robots), like the plant.  The EE position is three coalesced 512-byte loads of
// the step's exchange block (entries PlantArgs::ee0 names: x y z follow each other); the target record tgt[B][ndev][7] goes through
// the wave's target tile (osc_common.hpp: its contract), stored by a wave in which a lane moved its target.  Per-robot state is SoA
// [ndev][stride]; a per-robot table is [walk wave][dev][w][3][64] (a lane's waypoint: three coalesced loads), a shared one
// [dev][w][3].  The distance is float64 with every product and sum rounded on its own (no contraction): the host can repeat it.
//
// init = 1 (irlosc_set_waypoints): every device's state fresh (path_fresh), waypoint 0 into the targets of every listed device; no block is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irlosc.h"
#include "osc_common.hpp"

namespace irlosc {

struct PathState { int32_t* index; uint32_t* arrivals; int32_t* last_tick; };      // the paths' per-robot state: [ndev][stride] each
// One robot's fresh state of one device (o: its word of the device's plane; W: the device's waypoints, 0: not listed): what the init
// launch of irlosc_set_waypoints leaves, and a reset of episodes
__device__ __forceinline__ void path_fresh(PathState st, size_t o, int W) { st.index[o] = W > 0 ? 0 : -1; st.arrivals[o] = 0u; st.last_tick[o] = -1; }

struct WaypointArgs {
    const double* xside;      // the step's exchange block [walk wave][n_entries][64] (init: not read)
    void* tgt;                // [B][ndev][7] targets of the slot, record type: xyz of the listed devices in place
    PathState st;
    const double* table;      // per_robot: [walk wave][ndev][wmax][3][64], else [ndev][wmax][3]
    double thr2[IRLOSC_MAX_DEV];        // threshold^2
    int32_t count[IRLOSC_MAX_DEV];      // W_d (0: no list)
    int32_t ee0[IRLOSC_MAX_DEV];        // exchange entry of each device's EE x
    uint8_t loop[IRLOSC_MAX_DEV];
    int32_t B, ndev, stride, wmax, per_robot, n_entries, tick, init;
};

template <typename T>
__global__ __launch_bounds__(64) void osc_waypoint_kernel(const WaypointArgs a) {
    __shared__ T s_t[64 * IRLOSC_MAX_DEV * 7];      // the wave's target tile
    const int lane = threadIdx.x;
    const int b0 = (int)blockIdx.x * 64;
    const int nvalid = min(64, a.B - b0);           // robots of this wave
    const bool valid = lane < nvalid;
    const int row = a.ndev * 7;
    T* __restrict__ tg = (T*)a.tgt + (size_t)b0 * row;
    tgt_tile_load(s_t, tg, nvalid, row);
    bool moved = false;
    for (int d = 0; d < a.ndev; ++d) {
        const int W = a.count[d];
        const size_t so = (size_t)d * a.stride + b0 + lane;
        if (a.init && valid) path_fresh(a.st, so, W);
        if (W <= 0) continue;                       // (uniform over the launch)
        int idx = 0;
        bool reached = valid;
        if (!a.init) {
            reached = false;
            if (valid) {                            // idle lanes load nothing
                idx = a.st.index[so];
                const double* __restrict__ x = a.xside + ((size_t)blockIdx.x * a.n_entries + a.ee0[d]) * 64 + lane;
                const T* t = s_t + lane * row + d * 7;
                const double d0 = __dsub_rn(x[0], (double)t[0]), d1 = __dsub_rn(x[64], (double)t[1]), d2 = __dsub_rn(x[128], (double)t[2]);
                const double dist2 = __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
                reached = idx < W && dist2 < a.thr2[d];                      // NaN: not reached
            }
            if (reached) {
                a.st.arrivals[so] += 1u;
                a.st.last_tick[so] = a.tick;
                idx = idx + 1 < W ? idx + 1 : (a.loop[d] ? 0 : W);
                a.st.index[so] = idx;
            }
        }
        if (reached) {
            const int w = min(idx, W - 1);
            const size_t e = ((size_t)d * a.wmax + w) * 3;
            const double* __restrict__ p = a.per_robot ? a.table + ((size_t)blockIdx.x * a.ndev * a.wmax * 3 + e) * 64 + lane : a.table + e;
            const int cs = a.per_robot ? 64 : 1;
            T* t = s_t + lane * row + d * 7;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = (T)p[c * cs];
            moved = true;
        }
    }
    tgt_tile_store(tg, s_t, nvalid, row, moved);
}

}  // namespace irlosc
