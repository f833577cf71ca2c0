// Translation unit of the pack pass (osc_pack.hpp): dense records of a slot -> the compact block the lane-per-robot OSC step reads,
// and the host-side table of what goes where for the Dual-UR5 tree.
#include <algorithm>
#include <cstring>
#include <vector>

#include "osc_frontend_lane.hpp"
#include "osc_pack.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

bool pack_plan(const FeModel& h, PackTable* t) {
    using T = TopoDualUr5;
    using TI = FeTopo<T>;
    constexpr int NJ = T::NJ;
    const int nc = TI::n_compact(), nq = 2 * NJ, k = h.k, nd = h.ndev;
    if (h.nj != NJ || k < 1 || k > IRLOSC_MAX_K || nd < 1 || nd > IRLOSC_MAX_DEV) return false;
    std::vector<uint32_t> items;
    std::vector<int> written(nc + nq, 0);
    auto put = [&](uint32_t arr, int off, int e) { items.push_back(pack_item(arr, (uint32_t)off, (uint32_t)e)); ++written[e]; };
    auto check = [&](uint32_t arr, int off) { items.push_back(pack_item(arr, (uint32_t)off, PACK_CHECK)); };
    // M: pairs and diagonal from the lower triangle; the rest of the lower triangle must be zero (the upper one mirrors it: the
    // symmetry probe of the upload, or symmetric by construction)
    for (int r = 0; r < NJ; ++r)
        for (int c = 0; c <= r; ++c) {
            if (r == c) put(PACK_M, r * NJ + c, TI::diag_index(r));
            else if (TI::above(c, r)) put(PACK_M, r * NJ + c, TI::pair_index(c, r));
            else check(PACK_M, r * NJ + c);
        }
    // per device: the pose and the selected components of the Jacobian of its EE body; one device per body (the block holds one set
    // of entries per body: two devices' records of one body could disagree)
    std::vector<int> body_dev(T::NB, -1);
    for (int d = 0; d < nd; ++d) {
        const int b = h.ee_body[d];
        if (b < 0 || b >= T::NB || !T::ee_cand[b] || body_dev[b] >= 0) return false;
        body_dev[b] = d;
    }
    std::vector<int> jrow_seen(k, 0);
    for (int b = 0; b < T::NB; ++b) {
        if (!T::ee_cand[b]) continue;
        const int e0 = TI::ee_index(b), d = body_dev[b];
        if (d < 0) {      // a candidate no device names: zeros
            for (int e = 0; e < 7 + 6 * TI::n_above(b); ++e) put(PACK_ZERO, 0, e0 + e);
            continue;
        }
        for (int i = 0; i < 7; ++i) put(PACK_EE, d * 7 + i, e0 + i);
        int row = h.row0[d];
        for (int comp = 0; comp < 6; ++comp) {
            const bool sel = (h.dofmask[d] >> comp) & 1u;
            if (sel && (row < 0 || row >= k)) return false;
            for (int i = 0; i < NJ; ++i) {
                if (TI::moves(i, b)) {
                    const int e = e0 + 7 + 6 * TI::anc_rank(i, b) + comp;
                    if (sel) put(PACK_J, row * NJ + i, e);
                    else put(PACK_ZERO, 0, e);
                } else if (sel) {
                    check(PACK_J, row * NJ + i);
                }
            }
            if (sel) ++jrow_seen[row++];
        }
    }
    for (int r = 0; r < k; ++r) if (jrow_seen[r] != 1) return false;      // every row of J belongs to exactly one device
    for (int j = 0; j < NJ; ++j) put(PACK_BIAS, j, TI::bias_index(j));
    put(PACK_ZERO, 0, TI::zero_index());
    for (int r = 0; r < IRLOSC_MAX_K; ++r) put(PACK_ZERO, 0, TI::task_index(r));
    for (int j = 0; j < NJ; ++j) { put(PACK_ZERO, 0, nc + 2 * j); put(PACK_DQ, j, nc + 2 * j + 1); }
    for (int e = 0; e < nc + nq; ++e) if (written[e] != 1) return false;      // every output entry exactly once
    if ((int)items.size() > PACK_MAX_ITEMS) return false;
    std::sort(items.begin(), items.end());          // by (array, offset): each chunk of the records is brought in once
    memset(t, 0, sizeof *t);
    t->n_items = (int32_t)items.size();
    t->n_compact = nc;
    t->n_dq = nq;
    t->stride[PACK_M] = NJ * NJ;
    t->stride[PACK_J] = k * NJ;
    t->stride[PACK_DQ] = NJ;
    t->stride[PACK_BIAS] = NJ;
    t->stride[PACK_EE] = nd * 7;
    std::copy(items.begin(), items.end(), t->item);
    return true;
}

int pack_entries() { return FeTopo<TopoDualUr5>::n_compact(); }

// irlosc_time_trains on the lane route: the end of a train's OSC step is the end of its eigen pass (the row16 kernel's span holds its
// in-kernel eigen stage) -- stamped by one wave queued behind it (the slot-0 end of the train's span pairs: a max over the slots)
__global__ __launch_bounds__(64) void osc_span_end_kernel(unsigned long long* span) {
    if (threadIdx.x == 0) atomicMax(span + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

int launch_span_end(unsigned long long* span, hipStream_t st) {
    hipLaunchKernelGGL(osc_span_end_kernel, dim3(1), dim3(64), 0, st, span);
    return (int)hipGetLastError();
}

int launch_pack(const PackArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(osc_pack_kernel<PACK_CW>, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace irlosc
