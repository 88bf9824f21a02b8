// epipf_kernels_wide.hip -- the one-lane-per-particle kernels of the subgroup models at G = 5..8 (epipf_kernels.hpp;
// FastSubgroupsWide / SubgroupsStateWide, epipf_device.hpp), in a translation unit of their own for compile time.
// No lane-group or one-workgroup kernels exist for these G (epipf_api.cpp routes them here whatever N is).
#include "epipf_kernels.hpp"

namespace epipf {

template <int MODEL>
static hipError_t launch_wide_model(const StepArgs& a, int G, int obs, int n_chains, const FilterStreams& fs) {
    switch (G) {
        case 5: return launch_obs<MODEL, 5, 64>(a, obs, n_chains, fs);
        case 6: return launch_obs<MODEL, 6, 64>(a, obs, n_chains, fs);
        case 7: return launch_obs<MODEL, 7, 64>(a, obs, n_chains, fs);
        case 8: return launch_obs<MODEL, 8, 64>(a, obs, n_chains, fs);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_filter_wide(const StepArgs& a, int model, int G, int obs, int n_chains, const FilterStreams& fs) {
    if (a.wg != 64 || a.lanes > 1) return hipErrorInvalidValue;
    return model == kSubgroups ? launch_wide_model<kSubgroups>(a, G, obs, n_chains, fs)
                               : launch_wide_model<kSubgroups2>(a, G, obs, n_chains, fs);
}

// the SSA of both subgroup models is the same (they differ in what is observed)
hipError_t launch_simulate_wide(const SimArgs& a, int G, hipStream_t s) {
    switch (G) {
        case 5: sim_t<kSubgroups, 5>(a, s); break;
        case 6: sim_t<kSubgroups, 6>(a, s); break;
        case 7: sim_t<kSubgroups, 7>(a, s); break;
        case 8: sim_t<kSubgroups, 8>(a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_simulate_path_wide(const SimPathArgs& a, int G, hipStream_t s) {
    switch (G) {
        case 5: sim_path_t<kSubgroups, 5>(a, s); break;
        case 6: sim_path_t<kSubgroups, 6>(a, s); break;
        case 7: sim_path_t<kSubgroups, 7>(a, s); break;
        case 8: sim_path_t<kSubgroups, 8>(a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace epipf
