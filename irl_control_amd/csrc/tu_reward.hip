// Translation unit of the reward kernel of the rollout (osc_reward.hpp): float and double records.
#include "osc_reward.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_reward(const RewardArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(osc_reward_kernel<T>, dim3((a.B + 63) / 64), dim3(64), a.init ? 0 : reward_lds_bytes<T>(a), st, a);
    return (int)hipGetLastError();
}
template int launch_reward<float>(const RewardArgs&, hipStream_t);
template int launch_reward<double>(const RewardArgs&, hipStream_t);

}  // namespace irlosc
