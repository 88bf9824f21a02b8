// epipf_forecast_summary.hip -- forecast_summary_kernel (epipf_forecast_summary.hpp) for SIR, SEIR and the subgroup
// models up to G = 4, and the dispatch over model and G (as launch_forecast).
#include "epipf_forecast_summary.hpp"

namespace epipf {

// The day histograms (peak_day [H], extinct_day [H + 1], uint32) are counted per block in LDS up to this many bytes of
// dynamic LDS (the log table is static LDS beside them) and with global atomics beyond; `limit` overrides it
// (EPIPF_FORECAST_SUMMARY_LDS, for tests that run both sides at a small H).
constexpr size_t kForecastSummaryLdsDays = 32 * 1024;

bool forecast_summary_lds_days(int H, long long limit) {
    const size_t bound = limit < 0 ? kForecastSummaryLdsDays : std::min((size_t)limit, kForecastSummaryLdsDays);
    return sizeof(uint32_t) * (2 * (size_t)H + 1) <= bound;
}

// the SSA of both subgroup models is the same (they differ in what is observed)
hipError_t launch_forecast_summary(const ForecastSummaryArgs& a, int model, int G, hipStream_t s) {
    switch (model) {
        case kSIR: forecast_summary_t<kSIR, 1>(a, s); break;
        case kSEIR: forecast_summary_t<kSEIR, 1>(a, s); break;
        default:
            switch (G) {
                case 1: forecast_summary_t<kSubgroups, 1>(a, s); break;
                case 2: forecast_summary_t<kSubgroups, 2>(a, s); break;
                case 3: forecast_summary_t<kSubgroups, 3>(a, s); break;
                case 4: forecast_summary_t<kSubgroups, 4>(a, s); break;
                default: return launch_forecast_summary_wide(a, G, s);
            }
    }
    return hipGetLastError();
}

}  // namespace epipf
