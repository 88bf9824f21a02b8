// epipf_forecast_summary_wide.hip -- forecast_summary_kernel (epipf_forecast_summary.hpp) for the subgroup models at
// G = 5..8, whose rates sit in each draw's WideParam block behind the ChainParam array; a translation unit of its own
// for compile time.
#include "epipf_forecast_summary.hpp"

namespace epipf {

hipError_t launch_forecast_summary_wide(const ForecastSummaryArgs& a, int G, hipStream_t s) {
    switch (G) {
        case 5: forecast_summary_t<kSubgroups, 5>(a, s); break;
        case 6: forecast_summary_t<kSubgroups, 6>(a, s); break;
        case 7: forecast_summary_t<kSubgroups, 7>(a, s); break;
        case 8: forecast_summary_t<kSubgroups, 8>(a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace epipf
