// Translation unit of the episode kernel of the rollout (osc_episode.hpp): the compiled Dual-UR5 tree (its hinge count), float and
// double records.
#include "osc_episode.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_episodes(const EpisodeArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL((osc_episode_kernel<TopoDualUr5, T>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_episodes<float>(const EpisodeArgs&, hipStream_t);
template int launch_episodes<double>(const EpisodeArgs&, hipStream_t);

}  // namespace irlosc
