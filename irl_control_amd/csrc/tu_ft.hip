// Translation unit of the F/T sensor-feed wrench kernel (osc_ft.hpp), float and double records.
#include "osc_ft.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_ft_wrench(const FtTrain& tr, int nsteps, hipStream_t st) {
    if (nsteps <= 0 || tr.B <= 0) return 0;
    hipLaunchKernelGGL(osc_ft_wrench_kernel<T>, dim3((tr.B + 63) / 64, nsteps), dim3(64), 0, st, tr);
    return (int)hipGetLastError();
}
template int launch_ft_wrench<float>(const FtTrain&, int, hipStream_t);
template int launch_ft_wrench<double>(const FtTrain&, int, hipStream_t);

}  // namespace irlosc
