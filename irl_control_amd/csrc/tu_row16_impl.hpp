// The fp64-arithmetic row16 path on records of type IRLOSC_R16_TIN: the Dual-UR5 shapes with an instantiation of their own
// (R16ExactShapes, osc_row16.hpp) and the give-up pass.  One translation unit per record type (tu_row16_f64.hip, tu_row16_f32.hip).
#pragma once
#include "osc_generic.hpp"
#include "osc_row16.hpp"
#include "topo_dual_ur5.hpp"     // the fused path exists for the compiled tree shape (irlosc_set_model checks the model against it)
#include "launchers.hpp"

namespace irlosc {

// launch(R16Shape<k, ndev>{}) for the shape of the train.  -> the HIP status (hipErrorNotSupported: a shape without an instantiation
// that is not marked `padded` -- row16_kernel_exact and this dispatch read the same list, so it does not happen)
template <typename TIN, class Launch>
static int exact_dispatch(const Row16Train<TIN>& tr, Launch&& launch) {
    if (!row16_exact_shape(R16ExactShapes{}, tr.p[0].k, tr.p[0].ndev, launch)) return (int)hipErrorNotSupported;
    return (int)hipGetLastError();
}

// nsteps steps of equal batch size B (the steps of one train), blockIdx.y = step
// tree: every record of the train carries the zero pattern of the compiled Dual-UR5 tree (irlosc.hip keeps that verdict per
// slot) -- the factorisation then runs in the tree-structured form on the dense records.
template <typename TIN>
int launch_row16(const Row16Train<TIN>& tr, int nsteps, bool tree, hipStream_t st) {
    const KParams<TIN>& p = tr.p[0];
    if (p.B <= 0 || nsteps <= 0) return 0;
    const dim3 grid((p.B + 3) / 4, nsteps);
    // part 1 of the task signal as a pass of its own (osc_task_rows_dense_kernel; no rows buffer: computed in the kernel)
    if (tr.x[0].trows) {
        hipLaunchKernelGGL((osc_task_rows_dense_kernel<TIN>), dim3((p.B + 63) / 64, nsteps), dim3(64 * p.ndev), 0, st, tr);
        const int rc = (int)hipGetLastError();      // (not left to the sticky last-error: the main launch below would be queued behind a failed pass)
        if (rc) return rc;
    }
    if (p.padded)      // every other n = 25 layout: the KMAX-padded variants (tu_row16_pad_impl.hpp)
        return tree ? launch_row16_pad_tree<TIN>(tr, nsteps, st) : launch_row16_pad_dense<TIN>(tr, nsteps, st);
    if (tree)
        return exact_dispatch(tr, [&](auto s) {
            hipLaunchKernelGGL((osc_row16_kernel<decltype(s)::k, decltype(s)::ndev, TIN, 25, false, TopoDualUr5>), grid, dim3(64), 0, st, tr);
        });
    return exact_dispatch(tr, [&](auto s) { hipLaunchKernelGGL((osc_row16_kernel<decltype(s)::k, decltype(s)::ndev, TIN, 25>), grid, dim3(64), 0, st, tr); });
}

// The same train on the fused path: operands from the compact exchange buffers (tr.x[i].side / qvel / tables), the
// factorisation in the tree-structured form of the compiled Dual-UR5 shape.  Blocks of FOUR waves (256 threads): block x takes
// robots 16 (x % 4) .. of walk wave x / 4, i.e. one 128-byte line of every entry of that wave's exchange block.
template <typename TIN>
int launch_row16_fromq(const Row16Train<TIN>& tr, int nsteps, hipStream_t st) {
    const KParams<TIN>& p = tr.p[0];
    if (p.B <= 0 || nsteps <= 0) return 0;
    const int waves = (p.B + 63) / 64;
    const dim3 grid(waves * 4, nsteps), tgrid(waves, nsteps);      // the task pass first: one lane per robot, block = walk wave
    if (p.padded) return launch_row16_pad_fromq<TIN>(tr, nsteps, st);
    const int rc = exact_dispatch(tr, [&](auto s) {
        hipLaunchKernelGGL((osc_task_rows_fromq_kernel<decltype(s)::k, decltype(s)::ndev, TIN, TopoDualUr5>), tgrid, dim3(64 * decltype(s)::ndev), 0, st, tr);
    });
    if (rc) return rc;
    return exact_dispatch(tr, [&](auto s) {
        hipLaunchKernelGGL((osc_row16_kernel<decltype(s)::k, decltype(s)::ndev, TIN, 25, true, TopoDualUr5>), grid, dim3(256), 0, st, tr);
    });
}

// The generic kernel (Jacobi, fp64 arithmetic) over the give-up lists of a train; zeroes the counters `reset` points at.
template <typename TIN>
int launch_row16_worklist(const Row16Train<TIN>& tr, int nsteps, int32_t* reset, hipStream_t st) {
    const KParams<TIN>& p = tr.p[0];
    hipLaunchKernelGGL((osc_generic_worklist_kernel<double, TIN>), dim3(64, nsteps), dim3(64),
                       generic_smem_bytes<double>(p.n, p.k, p.ndev), st, tr, reset);
    return (int)hipGetLastError();
}

template int launch_row16<IRLOSC_R16_TIN>(const Row16Train<IRLOSC_R16_TIN>&, int, bool, hipStream_t);
template int launch_row16_fromq<IRLOSC_R16_TIN>(const Row16Train<IRLOSC_R16_TIN>&, int, hipStream_t);
template int launch_row16_worklist<IRLOSC_R16_TIN>(const Row16Train<IRLOSC_R16_TIN>&, int, int32_t*, hipStream_t);

#ifdef IRLOSC_R16_TREE_MASKS      // (one definition in the library)
void row16_tree_masks(uint32_t mrow[32], uint32_t* jcols) { r16::tree_structure_masks<TopoDualUr5>(mrow, jcols); }
#endif

}  // namespace irlosc
