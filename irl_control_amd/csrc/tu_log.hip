// Translation unit of the episode log of the rollout (osc_log.hpp), float and double records.
#include "osc_log.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_log(const LogArgs& a, hipStream_t st) {
    if (a.R <= 0 || !a.mask) return 0;
    int wmax = 1;      // the LDS tile: 64 x the widest channel of this launch
    for (int i = 0; i < LOG_CHANNELS; ++i)
        if ((a.mask >> i) & 1u) wmax = log_width(i, a.n, a.ndev, a.nobj, a.n_out) > wmax ? log_width(i, a.n, a.ndev, a.nobj, a.n_out) : wmax;
    hipLaunchKernelGGL(osc_log_kernel<T>, dim3((a.R + 63) / 64), dim3(64), (size_t)64 * wmax * sizeof(double), st, a);
    return (int)hipGetLastError();
}
template int launch_log<float>(const LogArgs&, hipStream_t);
template int launch_log<double>(const LogArgs&, hipStream_t);

}  // namespace irlosc
