// Dense records -> the compact block of a slot (the resident lane route of irlosc_step / irlosc_step_resident).
//
// The lane-per-robot OSC step (osc_lane.hpp) reads its operands from a block laid out [walk wave][entry][64 robots]: the structural
// non-zeros of M and J, the end-effector poses, the bias forces and an entry of zeros (FeTopo::pair_index .. zero_index, the exchange
// block of the fused path), and dq from a block in the walk's coordinate layout [walk wave][2 NJ][64 robots] (entry 2 j + 1 = dq_j).
// This pass builds both from the dense records of a slot ONCE, when the records enter it, so that every step after that reads
// 2.7 KB per robot in 512-byte wave loads instead of the 8.5 KB of row-major records.  It is the inverse of the record-form front
// end's epilogue (osc_frontend_lane.hpp): M pairs and diagonal from the lower triangle; per device, the EE pose and J's rows scattered
// to (component, ancestor rank) of the device's EE body; the bias forces; zeros everywhere else (components the layout does not
// select, EE candidates no device names, the entry of zeros, the task-row entries, the q entries of the dq block).
//
// What a robot drops on the way -- the lower triangle of M off the tree, the entries of J a row's hinges cannot move -- must be zero
// for the lane step to compute what the dense step computes; with `bad` given, the pass counts the robots where one is not.
//
// One wave per walk wave.  The source items are sorted by (array, offset) on the host; the wave walks them in that order and brings
// in each 32-double chunk of its 64 robots' records once: coalesced wave loads (two robots' 256-byte runs per instruction), transposed
// through LDS.  Every output entry is one 512-byte wave store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace irlosc {

enum : uint32_t { PACK_M = 0, PACK_J = 1, PACK_DQ = 2, PACK_BIAS = 3, PACK_EE = 4, PACK_N_ARR = 5, PACK_ZERO = 7 };
constexpr uint32_t PACK_CHECK = 0xFFF;        // item whose source must be zero (nothing is written)
constexpr int PACK_MAX_ITEMS = 1536;          // >= NJ^2 + IRLOSC_MAX_K NJ + 2 NJ + 7 IRLOSC_MAX_DEV + compact entries of the Dual-UR5
constexpr int PACK_CW = 32;                   // doubles per robot a chunk brings in

// item = array << 24 | offset << 12 | entry: entry < n_compact goes to the compact block, n_compact + e to entry e of the dq block
__host__ __device__ constexpr uint32_t pack_item(uint32_t arr, uint32_t off, uint32_t e) { return arr << 24 | off << 12 | e; }

struct PackTable {
    int32_t n_items;
    int32_t n_compact;        // entries per robot of the compact block
    int32_t n_dq;             // entries per robot of the dq block (2 NJ)
    int32_t stride[PACK_N_ARR];       // doubles per robot of M, J, dq, bias, ee_pose
    uint32_t item[PACK_MAX_ITEMS];
};

struct PackArgs {
    const PackTable* table;
    const double* src[PACK_N_ARR];    // the slot's dense records: M, J, dq, bias, ee_pose
    double* blk;                      // [wave][n_compact][64]
    double* dqb;                      // [wave][n_dq][64]
    int32_t* bad;                     // nullptr: no check
    int32_t B;
};

template <int CW>      // (a template only so that the header can be included by several translation units)
__global__ __launch_bounds__(64) void osc_pack_kernel(const PackArgs a) {
    __shared__ double tile[64 * (CW + 1)];       // [robot][chunk column], padded: conflict-free reads with the robot as the lane
    const PackTable* __restrict__ t = a.table;
    const int lane = threadIdx.x;
    const int inst0 = blockIdx.x * 64;
    const int nc = t->n_compact, nq = t->n_dq, n = t->n_items;
    double* __restrict__ blk = a.blk + (size_t)blockIdx.x * nc * 64 + lane;
    double* __restrict__ dqb = a.dqb + (size_t)blockIdx.x * nq * 64 + lane;
    uint32_t cur = ~0u;
    bool bad = false;
    for (int it = 0; it < n; ++it) {
        const uint32_t v = t->item[it];
        const uint32_t arr = v >> 24, off = (v >> 12) & 0xFFFu, e = v & 0xFFFu;
        double x = 0.0;
        if (arr < PACK_N_ARR) {
            const uint32_t ch = arr << 16 | off / CW;
            if (ch != cur) {      // the next chunk: 64 robots x CW doubles, all loads in flight together
                cur = ch;
                const double* __restrict__ s = a.src[arr];
                const int S = t->stride[arr];
                const int c0 = (int)(off / CW) * CW;
                double tv[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const int f = lane + 64 * i, r = f / CW, col = c0 + f % CW;
                    const int rb = min(inst0 + r, a.B - 1);       // idle lanes of a ragged last wave repeat the last robot
                    tv[i] = col < S ? s[(size_t)rb * S + col] : 0.0;
                }
                __syncthreads();                                   // the previous chunk's reads are done
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const int f = lane + 64 * i;
                    tile[(f / CW) * (CW + 1) + f % CW] = tv[i];
                }
                __syncthreads();
            }
            x = tile[lane * (CW + 1) + off % CW];
        }
        if (e == PACK_CHECK) bad |= x != 0.0;
        else if ((int)e < nc) blk[(size_t)e * 64] = x;
        else dqb[(size_t)(e - nc) * 64] = x;
    }
    if (a.bad && bad && inst0 + lane < a.B) atomicAdd(a.bad, 1);
}

}  // namespace irlosc
