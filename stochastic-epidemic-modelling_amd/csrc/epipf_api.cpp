// epipf_api.cpp -- the C ABI of libepipf.so (declared in include/epipf.h).
//
// A context owns every device buffer for one (model, G, N, t_max, max_chains) shape and one HIP
// stream; the observations, the log-factorial table and the whole particle history stay resident in
// HBM across calls, so an MH iteration moves only the chain parameters (host->device, ~200 B per
// chain) and the log-likelihoods + status (device->host) over PCIe.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/epipf.h"
#include "abc_device.hpp"
#include "epipf_if2.hpp"
#include "epipf_if2_sub.hpp"
#include "epipf_incidence.hpp"
#include "epipf_internal.hpp"
#include "epipf_smooth.hpp"
#include "epipf_smooth_lag.hpp"
#include "epipf_walk.hpp"
#include "epipf_walk_incidence.hpp"

using namespace epipf;

namespace {
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(EPIPF_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

template <class T>
int dalloc(T** p, size_t n) {
    if (n == 0) n = 1;
    if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        return fail(EPIPF_ENOMEM, "hipMalloc of %zu bytes failed", n * sizeof(T));
    }
    return 0;
}

int default_wg(int N) {
    // One wave per block at every N: the block-sum prefix is segmented (scan_segments), so a block's LDS does
    // not grow with N.
    (void)N;
    return 64;
}
}  // namespace

namespace epipf {
// the host MH draws (host_mh.cpp) report their argument errors through the same per-thread message
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace epipf

struct epipf_ctx {
    int device = 0, model = 0, G = 1, C = 3, K = 3, N = 0, Tmax = 0, max_chains = 0, wg = 64, B = 0;
    hipStream_t stream = nullptr;
    size_t hist_stride = 0, anc_stride = 0, wstride = 0, bstride = 0;
    int32_t *hidden = nullptr, *ancestry = nullptr, *status = nullptr, *chosen = nullptr, *traj = nullptr;
    // status [max_chains] | counters | log_zeta [max_chains][t_max] in one block (device and pinned host), so that a
    // run's results come back in one copy; status, counters and log_zeta point into it
    void* res = nullptr;
    void* h_res = nullptr;
    size_t res_counters = 0, res_lz = 0;   // byte offsets of counters and log_zeta in the block
    int32_t* h_traj = nullptr;             // pinned staging of epipf_run_sampled's trajectories
    double *wraw = nullptr, *wloc = nullptr, *bsum = nullptr, *log_zeta = nullptr, *Y = nullptr, *lf = nullptr;
    ChainParam* cp = nullptr;
    LogTab* logtab = nullptr;
    unsigned long long* counters = nullptr;
    // pinned staging
    ChainParam* h_cp = nullptr;
    int32_t* h_status = nullptr;
    double* h_lz = nullptr;
    unsigned long long* h_counters = nullptr;
    int T = 0, lf_max = -1, lf_cap = 0, last_chains = 0, last_T = 0;
    bool have_Y = false, have_pop = false, have_run = false;
    int profiling = 0;   // EPIPF_PROFILE_* level
    double npop[kMaxG] = {0}, mu[kMaxG] = {0}, emu[kMaxG] = {0};
    int kmax[kMaxG] = {0};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    epipf_stats stats{};
    // scratch for epipf_simulate / epipf_resample (grown on demand)
    size_t scratch_bytes = 0;
    void* scratch = nullptr;
    // ABC buffers (grown on demand): days, theta, dist for one batch; Y; accepted idx/count; output slots
    size_t abc_bytes = 0;
    void* abc = nullptr;
    bool abc_order = true;   // length-ordered ABC lanes (EPIPF_ABC_ORDER=0 disables)
    // lanes per trial for the longest ABC trials: 0 = automatic (abc_launch_trials), EPIPF_ABC_LANES overrides (1 = off)
    int abc_lanes = 0;
    double abc_frac = -1.0;  // share of the sorted trials on lane groups: < 0 automatic, EPIPF_ABC_GROUP_FRAC overrides
    bool fast_ssa = true;    // certified f32 event loop (EPIPF_SSA_FAST=0 disables; results are identical)
    bool seq_decide = false; // lane groups: the sequential decision pass instead of the fixed-point one
                             // (EPIPF_GROUP_DECIDE=seq; results are identical, A/B and tests)
    float clock_slack = 1.f; // EPIPF_CLOCK_SLACK >= 1 widens its clock band: replays on purpose (stress tests)
    float band_slack = 1.f;  // EPIPF_BAND_SLACK >= 1 widens the channel decision's band: exact decisions and redone
                             // lane-group chunks on purpose (stress tests)
    double tie_scale = 1.0;  // EPIPF_TIE_SCALE >= 1 widens particle_weight's tie band: the all-columns pass on purpose
    int n_streams = 4;   // chain groups on concurrent streams (EPIPF_STREAMS overrides, 1..kMaxFilterStreams)
    hipStream_t aux[kMaxFilterStreams] = {};
    hipEvent_t join[kMaxFilterStreams] = {};
    hipEvent_t fork = nullptr;
    hipEvent_t gb[kMaxFilterStreams] = {};   // per-group step spans (timing)
    hipEvent_t ge[kMaxFilterStreams] = {};
    int last_groups = 1;
    int lanes = 0;           // SSA lanes per particle: 0 = automatic (pick_lanes), else 1/2/4/8/16 (EPIPF_LANES)
    int lane_events = 0;     // events per lane per chunk of the lane-group kernel: 0 = automatic (EPIPF_LANE_EVENTS)
    int lane_blocks = 1280;  // automatic choice: lane groups up to this many particle blocks per launch
    int group_block = 0;     // lane-group runs' particles per block: 0 = automatic (pick_block), 16 or 64 (EPIPF_GROUP_BLOCK)
    int xcd_map = 1;         // XCD-aware placement of the step launches' blocks (EPIPF_XCD_MAP=0: 2-D grid)
    int group_lone = -1;     // lane-group runs' unbounded instance: -1 = by the launch's waves (pick_group_lone),
                             // 0 / 1 = never / wherever it exists (EPIPF_GROUP_LONE)
    // one-workgroup filter for N <= kFusedMaxN when the lanes are automatic: -1 = measured per batch size (FusedTune),
    // 1 = always, 0 = never (EPIPF_FUSED)
    int fused = -1;
    int fused_lanes = 0;     // its SSA lanes per particle: 0 = automatic (pick_fused), EPIPF_FUSED_LANES = 1/2/4/8/16
    uint64_t y_hash = 0;     // FNV-1a of the observations (epipf_set_observations): part of the path choice's key
    double split_p = -1.0;   // probs of the cached hi/lo split of log p, log1p(-p) (chains usually share probs)
    double split[4] = {0, 0, 0, 0};
    // the random-walk filter's parameter history (epipf_walk_filter): theta_hist [chains][T][d][N],
    // allocated on first use and regrown when a call needs more; walk_valid while it belongs to the context's history
    double* walk_theta = nullptr;
    size_t walk_bytes = 0;
    bool walk_valid = false;
    // incidence observations (epipf_run_incidence): the reports [D + 2][F] in a buffer of their own (Y is
    // not touched) and, for cumulated reports, the ping-pong accumulator int32 [2][chains][F][N]; both allocated on
    // first use and regrown when a call needs more.  acc_limit: a budget for the accumulator in bytes
    // (EPIPF_INCIDENCE_ACC_BYTES; 0: none), beyond which the call is EPIPF_ENOMEM without asking the device.
    double* inc_counts = nullptr;
    size_t inc_counts_n = 0;
    int32_t* inc_acc = nullptr;
    size_t inc_acc_bytes = 0, inc_acc_limit = 0;
    // negative-binomial reporting: the per-chain constants nb_coeff [chains][D + 2][F] and nb_chain
    // [chains][2] (kappa, log kappa), written by the host alone; allocated beside the counts buffer on first use and
    // regrown when a call needs more
    double* nb_coeff = nullptr;
    double* nb_chain = nullptr;
    size_t nb_coeff_n = 0, nb_chain_n = 0;
    // while the context's history is an incidence pass's (epipf_run_incidence, epipf_incidence_walk): what
    // epipf_incidence_smooth reduces
    bool inc_valid = false;
};

// Lanes per particle for a run of n_chains filters.  The one-lane kernel needs ~20k waves per launch to fill the
// chip; below 8 chains of 10^4 particles (n_chains x B <= 1280 particle blocks) the lane-group kernel with W = 4
// runs each particle-step 1.6-2.1x faster (1-8 chains, BASELINE configs 2 and 5: profiles/r2e_lanes_sweep*.jsonl;
// W = 2, 16 and K > 1 measured no better).  Up to 640 blocks (4 chains of 10^4) W = 8 is faster since round 3's
// mask-based decision pass and swizzle broadcasts (one chain: configs 2 / 3 / 5 +10% / +8% / +9%, four chains
// +3% / 0% / +9%; at 8 chains W = 4 leads by 16-29%: profiles/r3k_lanes_sweep_chains.jsonl).  Since round 4's
// fixed-point decision pass (a chunk's decisions cost ~2.3 evaluations instead of W dependent ones) and the clock pass
// through LDS, W = 16 leads up to two chains of 10^4 (320 blocks; one chain: configs 2 / 3 / 5 +12% / +16% / +18%
// over W = 8, two chains +9% / +10% / +12%), W = 8 from three (profiles/r4i_*, r4k_*).  With W = 16 on 16-particle
// blocks (pick_block) the subgroup models keep W = 16 up to four chains (+27% over W = 8 at three and four) and SIR /
// SEIR take W = 8 up to six (+11% / +7% over W = 4 at six; profiles/r4aa_lanes_sweep.txt).
static int pick_lanes(const epipf_ctx* c, int n_chains) {
    if (c->G > kMaxLaneG) return 1;                      // no lane-group kernels for G = 5..8 (epipf_kernels_wide.hip)
    if (c->lanes > 0) return c->lanes;
    const long blocks = (long)n_chains * c->B, lb = c->lane_blocks;
    if (c->model == EPIPF_SIR || c->model == EPIPF_SEIR)
        return blocks <= lb / 4 ? 16 : blocks <= lb * 3 / 4 ? 8 : blocks <= lb ? 4 : 1;
    // the W = 16 rule was measured on G = 2, whose decisions run as a fixed point (FastSubgroupsPacked::kFixedPoint,
    // G <= 2); G = 3, 4 keep the sequential pass (W dependent decisions per chunk) and round 3's W = 8
    if (c->G > 2) return blocks <= lb / 2 ? 8 : blocks <= lb ? 4 : 1;
    // round 5 (certified group clock): W = 16 leads up to six chains of 10^4 (+10% over W = 4 at six), W = 4 at eight
    // (profiles/r5l_lanes_pick_sweep.jsonl)
    return blocks <= lb * 3 / 4 ? 16 : blocks <= lb ? 4 : 1;
}

// Particles per block of a run's weight layout (block sums, in-block prefixes): 64, one wave of the one-lane kernel, or
// for W = 16 lane-group runs (at most two chains of 10^4, pick_lanes) kGroupBlock = 16 -- a chain of 10^4 particles is
// then 626 workgroups of 4 waves instead of 157 of 16 waves, spread over all 256 CUs.  Measured A/B
// (profiles/r4o_block_clock_ab.txt): W = 16, configs 2 / 3 / 5, one chain +1-2% / +4-6% / +18-20%, two chains 0-2% /
// 0-5% / +19%; at W = 8 the redundant block-sum scan per workgroup mostly costs more than the spread gains (-2% to -8%).
// EPIPF_GROUP_BLOCK = 16 / 64 forces either layout for W >= 8.
static int pick_block(const epipf_ctx* c, int W) {
    if (W < 8) return c->wg;
    if (c->group_block > 0) return c->group_block;
    return W >= 16 ? kGroupBlock : c->wg;
}

// The lane-group kernel's instance without the minimum-waves bound (epipf_group.hpp, group_lone_instance: subgroup
// models, G >= 2, W >= 8) when the launch's waves all stay resident at the unbounded kernel's occupancy -- 3 waves per
// SIMD at G = 2 (143 VGPRs), 2 at G = 3, 1 at G = 4 -- on the chip's 1024 SIMDs: BASELINE config 5's one chain of 10^4
// particles at W = 16 is 2,500 waves (2.4 per SIMD).  Larger launches keep the bounded instance (more waves resident, a
// few spills: +7% / +14% at two / four chains, profiles/README.md).
static int pick_group_lone(const epipf_ctx* c, const StepArgs& a, int n_chains) {
    if (a.lanes < 8 || c->model < EPIPF_SIR_SUBGROUPS || c->G < 2) return 0;
    if (c->group_lone >= 0) return c->group_lone;
    const long waves = (long)n_chains * a.B * ((long)a.wg * a.lanes / 64);
    const long per_simd = c->G == 2 ? 3 : c->G == 3 ? 2 : 1;
    return waves <= per_simd * 1024 ? 1 : 0;
}

// Lanes per particle of the one-workgroup filter (epipf_fused.hpp), or 0 when the run takes the step launches: N <=
// kFusedMaxN with the lanes automatic (an explicit epipf_set_lanes / EPIPF_LANES keeps the step kernels it names) and
// the chain's LDS within the default launch limit.  W: EPIPF_FUSED_LANES where its N W lanes fit one workgroup, else 1.
static int pick_fused(const epipf_ctx* c) {
    if (!c->fused || c->lanes > 0 || c->N > kFusedMaxN || c->G > kMaxLaneG) return 0;   // (no such kernel for G = 5..8)
    const int W = (c->fused_lanes > 0 && c->N * c->fused_lanes <= kFusedMaxThreads) ? c->fused_lanes : 1;
    if (fused_lds_bytes_of(c->N, c->C, fused_threads_of(c->N, W), 0, 0) > kFusedLdsLimit) return 0;
    return W;
}

// Which path is faster depends on the events per particle-step, which the host cannot see ahead: one workgroup per
// chain wins where a step is little work or many chains fill the chip (config 1, N = 100, 6 events: 3.1x at 256
// chains, 1.3x at one), the step launches where one chain's many events want more than one CU (N = 100 at config
// 2's 90 events: 2.2x the other way).  So a workload's first runs time both (the filter's device span, HIP events;
// results identical either way) and the faster one stays.
//
// The choice is PER PROCESS, keyed on the workload (device, model, observation model, N, T, chains per run, the
// observations and the population), not per context: contexts that run concurrently on one GPU (run_pipelined's chain
// groups) pool their timed runs into one decision and all take the same path.  Each context deciding alone from
// timings taken while the others ran let them settle on different paths.  A new dataset, T or population
// is a new key, so epipf_set_observations / epipf_set_population start a fresh choice.
struct FusedKey {
    int device, model, G, obs, N, T, n_chains;
    uint64_t data;
    bool operator<(const FusedKey& o) const {
        if (device != o.device) return device < o.device;
        if (model != o.model) return model < o.model;
        if (G != o.G) return G < o.G;
        if (obs != o.obs) return obs < o.obs;
        if (N != o.N) return N < o.N;
        if (T != o.T) return T < o.T;
        if (n_chains != o.n_chains) return n_chains < o.n_chains;
        return data < o.data;
    }
};
struct FusedTune {
    int issued = 0;                    // tuning runs handed out (they alternate the paths)
    int runs = 0;                      // tuning runs recorded
    double best[2] = {1e300, 1e300};   // fastest timed run: [0] step launches, [1] one-workgroup filter
    int choice = -1;
};
static std::mutex g_tune_mu;
static std::map<FusedKey, FusedTune> g_tune;

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

static FusedKey fused_key(const epipf_ctx* c, int obs, int n_chains) {
    const uint64_t h = fnv1a(c->y_hash, c->npop, sizeof(double) * c->G);
    return FusedKey{c->device, c->model, c->G, obs, c->N, c->T, n_chains, fnv1a(h, c->mu, sizeof(double) * c->G)};
}

// EPIPF_FUSED=auto (the default): the first 8 runs of a workload in this process alternate the paths (fused first, each
// path's first run untimed), then each path's fastest of three timed runs decides, the step launches only by a 15%
// margin (concurrent contexts share the device while they time, which spreads both paths' times).  *timed: this run's
// device span is recorded; *tuning: the choice is still open.
static bool fused_decide(const epipf_ctx* c, int obs, int n_chains, bool& timed, bool& tuning) {
    timed = tuning = false;
    if (c->fused >= 0) return c->fused == 1;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    FusedTune& t = g_tune[fused_key(c, obs, n_chains)];
    if (t.choice >= 0) return t.choice == 1;
    tuning = true;
    const int r = t.issued++;
    timed = r >= 2;                                      // runs 0, 1: warm-up of each path
    return (r & 1) == 0;                                 // even runs: fused
}

static void fused_record(const epipf_ctx* c, int obs, int n_chains, bool fused, double seconds) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    FusedTune& t = g_tune[fused_key(c, obs, n_chains)];
    t.best[fused ? 1 : 0] = std::min(t.best[fused ? 1 : 0], seconds);
    if (++t.runs >= 8 && t.choice < 0) t.choice = t.best[0] < 0.85 * t.best[1] ? 0 : 1;
}

static hipError_t launch_fused_run(const StepArgs& a, const epipf_ctx* c, int obs, int n_chains, const FilterStreams& fs) {
    const FusedFn f = fused_launcher(c->model, c->G, obs, a.lanes);
    if (!f) return hipErrorInvalidValue;
    const int threads = fused_threads_of(a.N, a.lanes);
    const size_t lds = fused_lds_bytes_of(a.N, c->C, threads, a.fused_y ? a.T * c->K : 0,
                                          a.fused_lf ? 2 * (a.lf_max + 1) : 0);
    const hipStream_t s = fs.s[0];
    if (fs.ev_init) (void)hipEventRecord(fs.ev_init, s);
    if (fs.ev_step0) (void)hipEventRecord(fs.ev_step0, s);    // init runs inside the one launch: its time is in step_ms
    if (fs.g_begin[0]) (void)hipEventRecord(fs.g_begin[0], s);
    EPIPF_RANGE_PUSH("one-workgroup filter");
    f(a, n_chains, threads, lds, s);
    EPIPF_RANGE_POP();
    if (fs.g_end[0]) (void)hipEventRecord(fs.g_end[0], s);
    if (fs.ev_end) (void)hipEventRecord(fs.ev_end, s);
    return hipGetLastError();
}

static int pick_lane_events(const epipf_ctx* c, int W) {
    if (W <= 1) return 1;
    if (c->lane_events > 0 && group_shape_supported(W, c->lane_events)) return c->lane_events;
    return 1;                                       // K > 1 measured no faster (profiles/r2e_lanes_sweep.jsonl)
}

// K = N + 2D + 8 of the resampling certificate (epipf_device.hpp): D bounds the depth of the parallel
// reduction tree behind every prefix: in-block scan (6 shuffle levels + <=4 wave offsets + 1) = 11 <= 16,
// block-sum scan 16 + 2 * ceil(B / WG) sequential chunk adds, +2 for the final adds.
static double cert_k(int N, int B, int S, int wg) {
    const int nseg = (B + S - 1) / S;
    const int per = ((nseg + wg - 1) / wg) * S;          // sequential block-sum adds per lane (scan_segments)
    const int D = 34 + 2 * per;
    return (double)N + 2.0 * D + 8.0;
}

// E: the relative error by which the reference's weights (scipy binom.pmf / norm.pdf) may differ from the device's.
// Binomial: scipy's Boost evaluation measured against 200-bit truth (scripts/scipy_pmf_envelope.py,
// profiles/r3_scipy_pmf_envelope.json: at most ~0.6 of this envelope over n <= 2e5, all p) plus the device's own
// <= 2 ulps; normal: numpy's exp vs the device's plus the divisions, 2^-48 (16 ulps).  An envelope, measured, not
// proven: the count it drives (resample_ref_ambiguous) is a diagnostic, never a decision.
static double ref_pmf_envelope(int obs_model, int n_max) {
    if (obs_model == EPIPF_OBS_NORMAL) return 0x1.0p-48;
    return 4e-12 + 1e-16 * (double)std::max(n_max, 0);
}

// parameter i of a chain: in ChainParam for the models up to kMaxLaneG groups, in the chain's WideParam block (w, or
// null) for the wider ones
static void set_theta(ChainParam& q, WideParam* w, int i, double v) {
    if (w) { w->theta[i] = v; w->thetaf[i] = (float)v; }
    else { q.theta[i] = v; q.thetaf[i] = (float)v; }
}

// ChainParam slots of an array of n chains' parameters: n, plus the room of n WideParam blocks behind them for a
// context with G > kMaxLaneG (wide_param, epipf_device.hpp)
static size_t cp_slots(int G, size_t n) {
    return n + (G > kMaxLaneG ? (n * sizeof(WideParam) + sizeof(ChainParam) - 1) / sizeof(ChainParam) : 0);
}
static_assert(sizeof(ChainParam) % alignof(WideParam) == 0, "WideParam blocks start behind a ChainParam array");
// one chain's parameters with its block, as epipf_simulate / epipf_simulate_path upload them
struct OneChain {
    ChainParam q;
    WideParam w;
};
static_assert(offsetof(OneChain, w) == sizeof(ChainParam), "wide_param(cp, 1, 0)");

static int theta_dim(int model, int G) { return model == EPIPF_SIR ? 2 : model == EPIPF_SEIR ? 3 : G * G + 1; }

static void free_ctx(epipf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void* dev[] = {c->hidden, c->ancestry, c->res, c->chosen, c->traj, c->wraw, c->wloc, c->bsum,
                   c->Y, c->lf, c->cp, c->logtab, c->scratch, c->abc, c->walk_theta, c->inc_counts, c->inc_acc,
                   c->nb_coeff, c->nb_chain};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    void* host[] = {c->h_cp, c->h_res, c->h_traj};
    for (void* p : host)
        if (p) (void)hipHostFree(p);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->join)
        if (e) (void)hipEventDestroy(e);
    for (int g = 0; g < kMaxFilterStreams; ++g) {
        if (c->gb[g]) (void)hipEventDestroy(c->gb[g]);
        if (c->ge[g]) (void)hipEventDestroy(c->ge[g]);
    }
    if (c->fork) (void)hipEventDestroy(c->fork);
    for (auto& st : c->aux)
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Streams and events of chain groups 0..n-1 (group 0 runs on c->stream), created on first use.
static bool ensure_streams(epipf_ctx* c, int n) {
    for (int g = 0; g < n; ++g) {
        if (!c->gb[g] && hipEventCreate(&c->gb[g]) != hipSuccess) return false;
        if (!c->ge[g] && hipEventCreate(&c->ge[g]) != hipSuccess) return false;
        if (g == 0) continue;
        if (!c->aux[g] && hipStreamCreateWithFlags(&c->aux[g], hipStreamNonBlocking) != hipSuccess) return false;
        if (!c->join[g] && hipEventCreateWithFlags(&c->join[g], hipEventDisableTiming) != hipSuccess) return false;
    }
    return true;
}

// The per-particle filters' inputs: half_widths [rows][d] and swarm [S][N][d], every entry finite and >= 0.
static int check_swarm(const double* half_widths, size_t rows, const double* swarm, size_t S, int N, int d) {
    for (size_t i = 0; i < rows * d; ++i)
        if (!(half_widths[i] >= 0.0 && half_widths[i] < INFINITY))
            return fail(EPIPF_EINVAL, "half_widths[%zu][%zu]=%g: half-widths must be finite and >= 0", i / d, i % d, half_widths[i]);
    for (size_t i = 0; i < S * N * d; ++i)
        if (!(swarm[i] >= 0.0 && swarm[i] < INFINITY))
            return fail(EPIPF_EINVAL, "swarm[%zu][%zu][%zu]=%g: parameters must be finite and >= 0", i / ((size_t)N * d),
                        i / d % N, i % d, swarm[i]);
    return EPIPF_OK;
}

// The fields of a filter launch's arguments that follow from the context alone: sizes, strides, tables, the context's
// own buffers and the constants of the initial-state draw.  The caller chooses the layout (wg, B, lanes, seg, nseg,
// cert_k) and the resampling mode.
static void step_args_of(const epipf_ctx* c, StepArgs& a) {
    a.N = c->N; a.T = c->T; a.max_chains = c->max_chains; a.lf_max = c->lf_max;
    a.count_events = c->profiling >= EPIPF_PROFILE_COUNTERS ? 1 : 0;
    a.hist_stride = c->hist_stride; a.anc_stride = c->anc_stride; a.wstride = c->wstride; a.bstride = c->bstride;
    a.Y = c->Y; a.lf = c->lf; a.logtab = c->logtab; a.cp = c->cp; a.hidden = c->hidden; a.ancestry = c->ancestry;
    a.wraw = c->wraw; a.wloc = c->wloc; a.bsum = c->bsum; a.log_zeta = c->log_zeta; a.status = c->status;
    a.counters = c->counters;
    a.xcd_map = c->xcd_map;
    for (int g = 0; g < kMaxLaneG; ++g) { a.npop[g] = c->npop[g]; a.mu[g] = c->mu[g]; a.emu[g] = c->emu[g]; a.kmax[g] = c->kmax[g]; }
}

// The same for the filters that always run one lane per particle on 64-particle blocks with multinomial resampling
// (iterated filtering, the random-walk filter, incidence observations), T rows long.
static void one_lane_step_args(const epipf_ctx* c, int T, StepArgs& s) {
    step_args_of(c, s);
    s.T = T; s.wg = 64; s.B = (c->N + 63) / 64; s.lanes = 1; s.lane_events = 1;
    s.resample_mode = EPIPF_RESAMPLE_MULTINOMIAL;
    s.seg = prefix_segment(s.B);
    s.nseg = (s.B + s.seg - 1) / s.seg;
    s.cert_k = cert_k(c->N, s.B, s.seg, 64);
}

// The streams of a run in n chain groups: group 0 on c->stream, where the groups' inputs are; the others wait for it.
// Created on first use, not with the context: HIP maps streams onto its few hardware queues in creation order, so
// contexts that each run one group (run_pipelined) get one stream each and land on different queues.
static int fork_streams(epipf_ctx* c, int n, FilterStreams& fs) {
    fs.n = n;
    if (!ensure_streams(c, fs.n)) return fail(EPIPF_EHIP, "auxiliary stream creation failed");
    fs.s[0] = c->stream;
    if (fs.n > 1) HIP_TRY(hipEventRecord(c->fork, c->stream));
    for (int g = 1; g < fs.n; ++g) {
        fs.s[g] = c->aux[g];
        fs.join[g] = c->join[g];
        HIP_TRY(hipStreamWaitEvent(c->aux[g], c->fork, 0));
    }
    c->last_groups = fs.n;
    return EPIPF_OK;
}

// The device counters of the last run, copied to c->h_counters, summed over their slots into the statistics.
// resample_fallbacks is counted at every profiling level.  epipf_run reports every counter as it stands (events and
// ambiguous both true); the other filters report the event counters only where their kernels counted them
// (count_events) and never touch resample_ref_ambiguous, which only the plain filter counts.
static void harvest_counters(epipf_ctx* c, bool events, bool ambiguous) {
    unsigned long long tot[kNumCounters] = {};
    for (int sl = 0; sl < kCounterSlots; ++sl)
        for (int k = 0; k < kNumCounters; ++k) tot[k] += c->h_counters[(size_t)sl * kCounterStride + k];
    c->stats.resample_fallbacks = (int64_t)tot[1];
    if (events) {
        c->stats.events = (int64_t)tot[0];
        c->stats.lane_iterations = (int64_t)tot[2];
        c->stats.wave_lane_slots = (int64_t)tot[3];
        c->stats.ssa_exact_lanes = (int64_t)tot[4];
        c->stats.ssa_exact_waves = (int64_t)tot[5];
    }
    if (ambiguous) c->stats.resample_ref_ambiguous = (int64_t)tot[6];
}

extern "C" {

const char* epipf_last_error(void) { return g_err.c_str(); }
int epipf_abi_version(void) { return EPIPF_ABI_VERSION; }
int epipf_max_groups(void) { return kMaxG; }
static_assert(kStatusOk == EPIPF_STATUS_OK && kStatusDegenerate == EPIPF_STATUS_DEGENERATE &&
              kStatusSkipped == EPIPF_STATUS_SKIPPED, "device status codes");
const char* epipf_build_id(void) {
#ifdef EPIPF_BUILD_ID
    return EPIPF_BUILD_ID;
#else
    return "unknown";
#endif
}
int epipf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int epipf_create(epipf_ctx** out, int device, int model, int groups, int n_particles, int t_max, int max_chains) {
    if (!out) return fail(EPIPF_EINVAL, "out is NULL");
    *out = nullptr;
    if (model < EPIPF_SIR || model > EPIPF_SIR_SUBGROUPS2) return fail(EPIPF_EINVAL, "unknown model %d", model);
    const int G = model >= EPIPF_SIR_SUBGROUPS ? groups : 1;
    if (G < 1 || G > kMaxG) return fail(EPIPF_EINVAL, "groups must be in [1, %d], got %d", kMaxG, groups);
    if (n_particles < 1 || t_max < 1 || max_chains < 1) return fail(EPIPF_EINVAL, "n_particles, t_max, max_chains must be >= 1");
    if (t_max > (1 << 24)) return fail(EPIPF_EINVAL, "t_max must be < 2^24 (Philox step field)");
    int ndev = epipf_device_count();
    if (device < 0 || device >= ndev) return fail(EPIPF_EINVAL, "device %d not present (%d HIP devices)", device, ndev);
    epipf_ctx* c = new epipf_ctx();
    c->device = device;
    c->model = model;
    c->G = G;
    c->C = model == EPIPF_SIR ? 3 : model == EPIPF_SEIR ? 4 : 3 * G;
    c->K = model == EPIPF_SIR_SUBGROUPS2 ? 3 : c->C;
    c->N = n_particles;
    c->Tmax = t_max;
    c->max_chains = max_chains;
    c->wg = default_wg(n_particles);
    if (const char* e = getenv("EPIPF_SSA_FAST")) c->fast_ssa = atoi(e) != 0;
    if (const char* e = getenv("EPIPF_GROUP_DECIDE")) c->seq_decide = strcmp(e, "seq") == 0;
    if (const char* e = getenv("EPIPF_CLOCK_SLACK")) c->clock_slack = std::max(1.0f, std::min(1e12f, (float)atof(e)));
    if (const char* e = getenv("EPIPF_BAND_SLACK")) c->band_slack = std::max(1.0f, std::min(1e4f, (float)atof(e)));
    if (const char* e = getenv("EPIPF_TIE_SCALE")) c->tie_scale = std::max(1.0, std::min(1e300, atof(e)));
    if (const char* e = getenv("EPIPF_INCIDENCE_ACC_BYTES")) c->inc_acc_limit = (size_t)std::max(0LL, atoll(e));
    if (const char* e = getenv("EPIPF_STREAMS")) c->n_streams = std::max(1, std::min(kMaxFilterStreams, atoi(e)));
    if (const char* e = getenv("EPIPF_LANES")) {
        const int w = atoi(e);
        if (w == 0 || w == 1 || w == 2 || w == 4 || w == 8 || w == 16) c->lanes = w;
        if (c->lanes > 1 && G > kMaxLaneG) {
            free_ctx(c);
            return fail(EPIPF_EINVAL, "EPIPF_LANES=%d with G=%d: lane groups exist for G <= %d", w, G, kMaxLaneG);
        }
    }
    if (const char* e = getenv("EPIPF_LANE_BLOCKS")) c->lane_blocks = std::max(0, atoi(e));
    if (const char* e = getenv("EPIPF_LANE_EVENTS")) c->lane_events = std::max(0, atoi(e));
    if (const char* e = getenv("EPIPF_GROUP_BLOCK")) {
        const int b = atoi(e);
        if (b == 0 || b == kGroupBlock || b == 64) c->group_block = b;
    }
    if (const char* e = getenv("EPIPF_XCD_MAP")) c->xcd_map = atoi(e) != 0;
    if (const char* e = getenv("EPIPF_GROUP_LONE")) c->group_lone = strcmp(e, "auto") == 0 ? -1 : atoi(e) != 0;
    if (const char* e = getenv("EPIPF_FUSED")) c->fused = strcmp(e, "auto") == 0 ? -1 : atoi(e) != 0;
    if (const char* e = getenv("EPIPF_FUSED_LANES")) {
        const int w = atoi(e);
        if (w == 0 || w == 1 || w == 2 || w == 4 || w == 8 || w == 16) c->fused_lanes = w;
    }
    c->B = (n_particles + c->wg - 1) / c->wg;
    if (step_lds_bytes(c->B, c->wg) > 160 * 1024) {
        free_ctx(c);
        return fail(EPIPF_EINVAL, "n_particles %d too large for one LDS block-sum table", n_particles);
    }
    c->hist_stride = (size_t)t_max * n_particles * c->C;
    c->anc_stride = (size_t)t_max * n_particles;
    c->wstride = (size_t)c->B * c->wg;
    // block sums for the lane-group runs' 16-particle blocks too (pick_block, kGroupBlock)
    c->bstride = std::max((size_t)c->B, (size_t)((n_particles + kGroupBlock - 1) / kGroupBlock));
    // and for the 64-particle one-wave blocks that iterated filtering forces at every model (if2_impl: wg = 64,
    // lanes = 1), whatever default_wg and the lane-group runs pick; today default_wg is 64, so these change nothing
    const size_t B64 = ((size_t)n_particles + 63) / 64;
    c->wstride = std::max(c->wstride, B64 * 64);
    c->bstride = std::max(c->bstride, B64);
    int rc = 0;
    if (hipSetDevice(device) != hipSuccess) { free_ctx(c); return fail(EPIPF_EHIP, "hipSetDevice(%d) failed", device); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        free_ctx(c);
        return fail(EPIPF_EHIP, "hipStreamCreate failed");
    }
    rc |= dalloc(&c->hidden, (size_t)max_chains * c->hist_stride);
    rc |= dalloc(&c->ancestry, (size_t)max_chains * c->anc_stride);
    c->res_counters = ((sizeof(int32_t) * (size_t)max_chains + 127) / 128) * 128;
    c->res_lz = c->res_counters + sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride;
    const size_t res_bytes = c->res_lz + sizeof(double) * (size_t)max_chains * t_max;
    rc |= dalloc(reinterpret_cast<char**>(&c->res), res_bytes);
    rc |= dalloc(&c->chosen, (size_t)max_chains);
    rc |= dalloc(&c->traj, (size_t)max_chains * t_max * c->C);
    rc |= dalloc(&c->wraw, 2 * (size_t)max_chains * c->wstride);
    rc |= dalloc(&c->wloc, 2 * (size_t)max_chains * c->wstride);
    rc |= dalloc(&c->bsum, 2 * (size_t)max_chains * c->bstride);
    rc |= dalloc(&c->cp, cp_slots(G, (size_t)max_chains));
    rc |= dalloc(&c->logtab, (size_t)kLogTabEntries);
    if (rc) { free_ctx(c); return EPIPF_ENOMEM; }
    c->status = static_cast<int32_t*>(c->res);
    c->counters = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->res) + c->res_counters);
    c->log_zeta = reinterpret_cast<double*>(static_cast<char*>(c->res) + c->res_lz);
    if (hipHostMalloc((void**)&c->h_cp, sizeof(ChainParam) * cp_slots(G, (size_t)max_chains)) != hipSuccess ||
        hipHostMalloc(&c->h_res, res_bytes) != hipSuccess ||
        hipHostMalloc((void**)&c->h_traj, sizeof(int32_t) * (size_t)max_chains * t_max * c->C) != hipSuccess) {
        free_ctx(c);
        return fail(EPIPF_ENOMEM, "hipHostMalloc failed");
    }
    c->h_status = static_cast<int32_t*>(c->h_res);
    c->h_counters = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->h_res) + c->res_counters);
    c->h_lz = reinterpret_cast<double*>(static_cast<char*>(c->h_res) + c->res_lz);
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) { free_ctx(c); return fail(EPIPF_EHIP, "hipEventCreate failed"); }
    if (hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) != hipSuccess) {
        free_ctx(c);
        return fail(EPIPF_EHIP, "hipEventCreate failed");
    }
    // on the context stream (a NULL-stream copy would take one of the process's hardware queues, which the
    // chain-group streams then share: two groups serialised, -14% at config 2)
    LogTab lt[kLogTabEntries];                 // synchronised below, before it goes out of scope
    glibc_log_table(lt);
    if (hipMemcpyAsync(c->logtab, lt, sizeof lt, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        free_ctx(c);
        return fail(EPIPF_EHIP, "counter init failed");
    }
    *out = c;
    return EPIPF_OK;
}

void epipf_destroy(epipf_ctx* ctx) { free_ctx(ctx); }

int epipf_set_observations(epipf_ctx* c, const double* Y, int T, int K) {
    if (!c || !Y) return fail(EPIPF_EINVAL, "NULL argument");
    if (T < 1 || T > c->Tmax) return fail(EPIPF_EINVAL, "T=%d outside [1, t_max=%d]", T, c->Tmax);
    if (K != c->K) return fail(EPIPF_EINVAL, "K=%d but the model observes %d columns", K, c->K);
    HIP_TRY(hipSetDevice(c->device));
    if (c->Y) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->Y); c->Y = nullptr; }
    if (dalloc(&c->Y, (size_t)T * K)) return EPIPF_ENOMEM;
    HIP_TRY(hipMemcpyAsync(c->Y, Y, sizeof(double) * (size_t)T * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->T = T;
    c->y_hash = fnv1a(0xcbf29ce484222325ull ^ (uint64_t)T, Y, sizeof(double) * (size_t)T * K);
    c->have_Y = true;
    return EPIPF_OK;
}

int epipf_set_population(epipf_ctx* c, const double* n_population, const double* mu) {
    if (!c || !n_population || !mu) return fail(EPIPF_EINVAL, "NULL argument");
    double tot = 0.0;
    for (int g = 0; g < c->G; ++g) {
        const double np_ = n_population[g], m = mu[g];
        if (!(np_ >= 0.0) || np_ != std::floor(np_) || np_ > 1e8)
            return fail(EPIPF_EINVAL, "n_population[%d]=%g must be an integer in [0, 1e8]", g, np_);
        if (!(m >= 0.0) || m > 700.0) return fail(EPIPF_EINVAL, "mu[%d]=%g must be in [0, 700]", g, m);
        c->npop[g] = np_;
        c->mu[g] = m;
        c->emu[g] = std::exp(-m);                                        // host glibc, as the oracle
        c->kmax[g] = (int)std::ceil(m + 40.0 * std::sqrt(m) + 60.0);
        tot += np_;
    }
    const int need = (int)tot;
    HIP_TRY(hipSetDevice(c->device));
    if (need + 1 > c->lf_cap) {
        if (c->lf) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->lf); c->lf = nullptr; }
        if (dalloc(&c->lf, 2 * ((size_t)need + 1))) return EPIPF_ENOMEM;
        c->lf_cap = need + 1;
    }
    if (need != c->lf_max) {
        std::vector<double> lf(2 * ((size_t)need + 1));
        logfact_table(need, lf.data());                      // log n!: hi parts, then lo parts (binom_logpmf)
        HIP_TRY(hipMemcpyAsync(c->lf, lf.data(), sizeof(double) * lf.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->lf_max = need;
    }
    c->have_pop = true;
    return EPIPF_OK;
}

// What a chain's filter needs besides theta: the observation parameter with its binary128 log splits, the weight's tie
// tolerance, the Philox key and filter index, and the context's SSA switches (epipf_run, epipf_if2).
static void set_chain_stream(epipf_ctx* c, ChainParam& q, double probs, uint64_t key, uint32_t f) {
    q.probs = probs;
    if (!(probs == c->split_p) && !(std::isnan(probs) && std::isnan(c->split_p))) {   // binary128: ~2 us
        log_p_split(probs, &c->split[0], &c->split[1], &c->split[2], &c->split[3]);
        c->split_p = probs;
    }
    q.logp = c->split[0]; q.logp_lo = c->split[1]; q.log1mp = c->split[2]; q.log1mp_lo = c->split[3];
    // particle_weight's tie tolerance: 8x a bound on its plain column logs' error, ~8 roundings of at most half
    // an ulp of the sum of their terms' magnitudes, 2 log n! + n (|log p| + |log1p(-p)|) at n = the population
    const double nmax = (double)std::max(c->lf_max, 0);
    q.tie_tol = (2.0 * std::lgamma(nmax + 1.0) * 1.01 + nmax * (std::fabs(q.logp) + std::fabs(q.log1mp)) + 1.0) *
                0x1.0p-46 * c->tie_scale;
    q.k0 = (uint32_t)key;
    q.k1 = (uint32_t)(key >> 32);
    q.f = f;
    q.flags = (c->fast_ssa ? kChainFastSsa : 0u) | (c->seq_decide ? kChainSeqDecide : 0u);
    q.clock_slack = c->clock_slack;
    q.band_slack = c->band_slack;
}

static int run_impl(epipf_ctx* c, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                    const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, int resample_mode,
                    const int32_t* chosen, double* log_zetas_out, int32_t* status_out, int32_t* traj_out) {
    if (!c || !theta || !probs || !keys || !filter_index || !status_out) return fail(EPIPF_EINVAL, "NULL argument");
    if ((chosen == nullptr) != (traj_out == nullptr)) return fail(EPIPF_EINVAL, "chosen and traj_out go together");
    if (!c->have_Y) return fail(EPIPF_ESTATE, "epipf_set_observations was not called");
    if (!c->have_pop) return fail(EPIPF_ESTATE, "epipf_set_population was not called");
    if (n_chains < 1 || n_chains > c->max_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->max_chains);
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta has %d entries per chain, model needs %d", d, theta_dim(c->model, c->G));
    if (obs_model != EPIPF_OBS_BINOMIAL && obs_model != EPIPF_OBS_NORMAL) return fail(EPIPF_EINVAL, "bad obs_model %d", obs_model);
    if (resample_mode != EPIPF_RESAMPLE_MULTINOMIAL && resample_mode != EPIPF_RESAMPLE_SYSTEMATIC)
        return fail(EPIPF_EINVAL, "bad resample_mode %d", resample_mode);
    int n_active = 0;
    for (int ch = 0; ch < n_chains; ++ch) {
        const bool on = !active || active[ch];
        ChainParam& q = c->h_cp[ch];
        memset(&q, 0, sizeof q);
        WideParam* w = c->G > kMaxLaneG ? const_cast<WideParam*>(wide_param(c->h_cp, c->max_chains, ch)) : nullptr;
        if (w) memset(w, 0, sizeof *w);
        for (int i = 0; i < d; ++i) {
            const double v = theta[(size_t)ch * d + i];
            if (on && !(v >= 0.0 && v < INFINITY))
                return fail(EPIPF_EINVAL, "theta[%d][%d]=%g: parameters must be finite and >= 0 (pmcmc.py:333)", ch, i, v);
            set_theta(q, w, i, v);
        }
        set_chain_stream(c, q, probs[ch], keys[ch], filter_index[ch]);
        for (int g = kMaxLaneG; w && g < kMaxG; ++g) {
            const int h = g - kMaxLaneG;
            w->npop_hi[h] = c->npop[g]; w->mu_hi[h] = c->mu[g]; w->emu_hi[h] = c->emu[g]; w->kmax_hi[h] = c->kmax[g];
        }
        q.skip = on ? 0 : 1;                            // the first kernel writes the chain's status from it
        q.chosen = -1;
        if (chosen && on) {
            if (chosen[ch] >= c->N) return fail(EPIPF_EINVAL, "chosen[%d]=%d outside [0, N)", ch, chosen[ch]);
            q.chosen = chosen[ch] < 0 ? -1 : chosen[ch];
        }
        n_active += on;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->walk_valid = false;                               // the history is this run's from here on
    c->inc_valid = false;
    HIP_TRY(hipMemcpyAsync(c->cp, c->h_cp, sizeof(ChainParam) * n_chains, hipMemcpyHostToDevice, c->stream));
    if (c->G > kMaxLaneG)   // the chains' WideParam blocks, behind the ChainParam array on both sides
        HIP_TRY(hipMemcpyAsync(const_cast<WideParam*>(wide_param(c->cp, c->max_chains, 0)), wide_param(c->h_cp, c->max_chains, 0),
                               sizeof(WideParam) * n_chains, hipMemcpyHostToDevice, c->stream));

    StepArgs a{};
    step_args_of(c, a);
    bool tune_timed = false, tuning = false;
    const int fusedW = pick_fused(c) && fused_decide(c, obs_model, n_chains, tune_timed, tuning) ? pick_fused(c) : 0;
    a.lanes = fusedW ? fusedW : pick_lanes(c, n_chains);
    a.wg = fusedW ? 64 : pick_block(c, a.lanes);
    a.B = (c->N + a.wg - 1) / a.wg;
    a.group_lone = fusedW ? 0 : pick_group_lone(c, a, n_chains);
    a.resample_mode = resample_mode;
    // S blocks per prefix segment: 1 (every block sum in LDS) for lane-group runs on 16-particle blocks up to
    // kMaxFlatGroupBlocks, else the smallest power of two with at most kMaxSegments segments
    // The 16-particle layout sums the step total in the 64-particle layout's order (scan_block_sums16): its segments are
    // whole segments of that layout (S16 = 4 S64, the same as prefix_segment(B16) wherever it segments), and canon_per
    // is that layout's 64-blocks per lane, so the log-likelihood is the same whichever layout the chain count picks.
    const int B64 = (c->N + 63) / 64, S64 = prefix_segment(B64);
    a.canon_per = ((B64 + S64 - 1) / S64 + 63) / 64 * S64;
    a.seg = fusedW ? 1 : (a.lanes > 1 && a.wg == kGroupBlock) ? (a.B <= kMaxFlatGroupBlocks ? 1 : 4 * S64) : prefix_segment(a.B);
    a.nseg = (a.B + a.seg - 1) / a.seg;
    a.cert_k = cert_k(c->N, a.B, a.seg, 64);              // the block-sum scans run on 64 lanes whatever the layout
    // the reference-ambiguity test runs with the other device counters (bench.py's untimed counters iteration, the
    // parity tests); ref_k = 0 switches it off in the timed, production launches
    a.ref_k = a.count_events ? 2.0 * ref_pmf_envelope(obs_model, c->lf_max) * (1.0 + 0x1.0p-10) : 0.0;
    a.lane_events = pick_lane_events(c, a.lanes);
    if (a.lanes > 1 && !group_shape_supported(a.lanes, a.lane_events))
        return fail(EPIPF_EINVAL, "no lane-group kernel for %d lanes x %d events", a.lanes, a.lane_events);
    c->stats.last_lanes = a.lanes;
    c->stats.last_lane_events = a.lane_events;
    c->stats.last_fused = fusedW ? 1 : 0;
    if (fusedW) {   // stage Y, then the log n! table, in LDS while the launch stays within the default dynamic LDS limit
        const int threads = fused_threads_of(a.N, a.lanes);
        const size_t base = fused_lds_bytes_of(a.N, c->C, threads, 0, 0);
        const size_t yb = sizeof(double) * (size_t)a.T * c->K, lb = sizeof(double) * 2 * (size_t)(a.lf_max + 1);
        a.fused_y = base + yb <= kFusedLdsLimit;
        a.fused_lf = a.lf_max >= 0 && base + (a.fused_y ? yb : 0) + lb <= kFusedLdsLimit;
    }

    EPIPF_RANGE_PUSH("epipf_run");
    struct RangeEnd { ~RangeEnd() { EPIPF_RANGE_POP(); } } range_end;
    FilterStreams fs{};
    if (const int e = fork_streams(c, fusedW ? 1 : std::min(c->n_streams, n_chains), fs)) return e;
    fs.ev_init = (c->profiling || tuning) ? c->ev[0] : nullptr;   // the path choice times the device span
    fs.ev_step0 = c->profiling ? c->ev[1] : nullptr;
    fs.ev_end = (c->profiling || tuning) ? c->ev[2] : nullptr;
    for (int g = 0; g < fs.n; ++g) {
        fs.g_begin[g] = c->profiling ? c->gb[g] : nullptr;
        fs.g_end[g] = c->profiling ? c->ge[g] : nullptr;
    }
    hipError_t le = fusedW ? launch_fused_run(a, c, obs_model, n_chains, fs)
                           : launch_filter(a, c->model, c->G, obs_model, n_chains, fs);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
    if (chosen) {   // the path sampler (pmcmc.py:236-248) after the filter, on the same stream: no second round trip
        PathArgs pa{};
        pa.n_chains = n_chains; pa.N = c->N; pa.T = c->T; pa.C = c->C;
        pa.hist_stride = c->hist_stride; pa.anc_stride = c->anc_stride;
        pa.hidden = c->hidden; pa.ancestry = c->ancestry; pa.chosen = nullptr; pa.cp = c->cp; pa.status = c->status;
        pa.traj = c->traj;
        hipError_t pe = launch_path_sample(pa, c->stream);
        if (pe != hipSuccess) return fail(EPIPF_EHIP, "path kernel launch failed: %s", hipGetErrorString(pe));
        HIP_TRY(hipMemcpyAsync(c->h_traj, c->traj, sizeof(int32_t) * (size_t)n_chains * c->T * c->C,
                               hipMemcpyDeviceToHost, c->stream));
    }
    // status, counters and the log-likelihoods: one copy of the result block's prefix
    HIP_TRY(hipMemcpyAsync(c->h_res, c->res, c->res_lz + sizeof(double) * (size_t)n_chains * c->T, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (tuning) {   // the filter's device span, init to the last step (host threads contending for the GIL do not
                    // enter it, as they would a wall clock)
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[2]));
        fused_record(c, obs_model, n_chains, fusedW != 0, tune_timed ? (double)ms : 1e300);
    }
    if (chosen) memcpy(traj_out, c->h_traj, sizeof(int32_t) * (size_t)n_chains * c->T * c->C);
    memcpy(status_out, c->h_status, sizeof(int32_t) * n_chains);
    if (log_zetas_out) {
        memcpy(log_zetas_out, c->h_lz, sizeof(double) * (size_t)n_chains * c->T);
        // steps after a degenerate step were never run: report -inf there (zetas = 0)
        for (int ch = 0; ch < n_chains; ++ch) {
            if (c->h_status[ch] == EPIPF_STATUS_OK) continue;
            bool dead = false;
            for (int p = 0; p < c->T; ++p) {
                double& v = log_zetas_out[(size_t)ch * c->T + p];
                if (c->h_status[ch] == EPIPF_STATUS_SKIPPED) { v = NAN; continue; }
                if (dead) v = -INFINITY;
                else if (v == -INFINITY) dead = true;
            }
        }
    }
    if (c->profiling) {
        float ms_init = 0.f, ms_step = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_init, c->ev[0], c->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_step, c->ev[1], c->ev[2]));
        c->stats.init_ms += ms_init;
        c->stats.init_launches += 1;
        c->stats.step_ms += ms_step;
        c->stats.step_launches += fusedW ? 1 : c->T - 1;   // the one-workgroup filter: one launch per run
        for (int g = 0; g < c->last_groups; ++g) {        // each group's back-to-back step kernels on its stream
            float ms_g = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms_g, c->gb[g], c->ge[g]));
            c->stats.step_kernel_ms += ms_g;
            c->stats.step_kernel_launches += fusedW ? 1 : c->T - 1;
        }
    }
    harvest_counters(c, true, true);
    c->stats.particle_steps += (int64_t)n_active * c->N * c->T;
    c->stats.filters += n_active;
    c->last_chains = n_chains;
    c->last_T = c->T;
    c->have_run = true;
    return EPIPF_OK;
}

int epipf_run(epipf_ctx* c, int n_chains, const double* theta, int d, int obs_model, const double* probs,
              const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, int resample_mode,
              double* log_zetas_out, int32_t* status_out) {
    return run_impl(c, n_chains, theta, d, obs_model, probs, keys, filter_index, active, resample_mode, nullptr,
                    log_zetas_out, status_out, nullptr);
}

int epipf_run_sampled(epipf_ctx* c, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                      const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, int resample_mode,
                      const int32_t* chosen, double* log_zetas_out, int32_t* status_out, int32_t* traj_out) {
    if (!chosen || !traj_out) return fail(EPIPF_EINVAL, "NULL argument");
    return run_impl(c, n_chains, theta, d, obs_model, probs, keys, filter_index, active, resample_mode, chosen,
                    log_zetas_out, status_out, traj_out);
}

int epipf_copy_history(epipf_ctx* c, int n_chains, int32_t* hidden_out, int32_t* ancestry_out) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (!c->have_run) return fail(EPIPF_ESTATE, "no filter has run on this context");
    if (n_chains < 1 || n_chains > c->last_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->last_chains);
    HIP_TRY(hipSetDevice(c->device));
    const size_t T = (size_t)c->last_T;
    if (hidden_out)
        HIP_TRY(hipMemcpy2DAsync(hidden_out, T * c->N * c->C * sizeof(int32_t), c->hidden, c->hist_stride * sizeof(int32_t),
                                 T * c->N * c->C * sizeof(int32_t), n_chains, hipMemcpyDeviceToHost, c->stream));
    if (ancestry_out)
        HIP_TRY(hipMemcpy2DAsync(ancestry_out, T * c->N * sizeof(int32_t), c->ancestry, c->anc_stride * sizeof(int32_t),
                                 T * c->N * sizeof(int32_t), n_chains, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EPIPF_OK;
}

int epipf_path_sample(epipf_ctx* c, int n_chains, const int32_t* chosen, int32_t* traj_out) {
    if (!c || !chosen || !traj_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (!c->have_run) return fail(EPIPF_ESTATE, "no filter has run on this context");
    if (n_chains < 1 || n_chains > c->last_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->last_chains);
    for (int ch = 0; ch < n_chains; ++ch)
        if (chosen[ch] < 0 || chosen[ch] >= c->N) return fail(EPIPF_EINVAL, "chosen[%d]=%d outside [0, N)", ch, chosen[ch]);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->chosen, chosen, sizeof(int32_t) * n_chains, hipMemcpyHostToDevice, c->stream));
    PathArgs a{};
    a.n_chains = n_chains; a.N = c->N; a.T = c->last_T; a.C = c->C;
    a.hist_stride = c->hist_stride; a.anc_stride = c->anc_stride;
    a.hidden = c->hidden; a.ancestry = c->ancestry; a.chosen = c->chosen; a.cp = c->cp; a.status = c->status;
    a.traj = c->traj;
    hipError_t le = launch_path_sample(a, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "path kernel launch failed: %s", hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(traj_out, c->traj, sizeof(int32_t) * (size_t)n_chains * a.T * a.C, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EPIPF_OK;
}

static int ensure_scratch(epipf_ctx* c, size_t bytes) {
    if (bytes <= c->scratch_bytes) return 0;
    if (c->scratch) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    if (hipMalloc(&c->scratch, bytes) != hipSuccess) return fail(EPIPF_ENOMEM, "scratch hipMalloc(%zu) failed", bytes);
    c->scratch_bytes = bytes;
    return 0;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Scratch above this stays allocated only for the call that needed it (a one-off long full-path batch must not pin
// gigabytes on a context get_engine caches for the whole process); the stream is synchronised by then.
constexpr size_t kScratchKeepBytes = (size_t)64 << 20;
static void trim_scratch(epipf_ctx* c) {
    if (c->scratch && c->scratch_bytes > kScratchKeepBytes) {
        (void)hipFree(c->scratch);
        c->scratch = nullptr;
        c->scratch_bytes = 0;
    }
}

int epipf_simulate(epipf_ctx* c, int n, const int32_t* states_in, const double* theta, int d, double max_time,
                   uint64_t key, uint32_t filter_index, uint32_t step, int32_t* states_out, int64_t* events_out) {
    if (!c || !states_in || !theta || !states_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 0) return fail(EPIPF_EINVAL, "n < 0");
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta needs %d entries", theta_dim(c->model, c->G));
    if (!(max_time >= 0.0)) return fail(EPIPF_EINVAL, "max_time must be >= 0");
    for (int i = 0; i < d; ++i)
        if (!(theta[i] >= 0.0 && theta[i] < INFINITY)) return fail(EPIPF_EINVAL, "theta[%d] must be finite and >= 0", i);
    for (size_t i = 0; i < (size_t)n * c->C; ++i)
        if (states_in[i] < 0) return fail(EPIPF_EINVAL, "states must be non-negative");
    if (n == 0) { if (events_out) *events_out = 0; return EPIPF_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t sb = align256((size_t)n * c->C * sizeof(int32_t));
    const size_t need = align256(sizeof(OneChain)) + 2 * sb + 256;
    if (ensure_scratch(c, need)) return EPIPF_ENOMEM;
    char* base = (char*)c->scratch;
    ChainParam* dcp = (ChainParam*)base;
    int32_t* din = (int32_t*)(base + align256(sizeof(OneChain)));
    int32_t* dout = (int32_t*)((char*)din + sb);
    unsigned long long* dev_events = (unsigned long long*)((char*)dout + sb);
    OneChain one;
    memset(&one, 0, sizeof one);
    ChainParam& q = one.q;
    for (int i = 0; i < d; ++i) set_theta(q, c->G > kMaxLaneG ? &one.w : nullptr, i, theta[i]);
    q.k0 = (uint32_t)key; q.k1 = (uint32_t)(key >> 32); q.f = filter_index;
    q.flags = (c->fast_ssa ? kChainFastSsa : 0u) | (c->seq_decide ? kChainSeqDecide : 0u);
    q.clock_slack = c->clock_slack;
    q.band_slack = c->band_slack;
    HIP_TRY(hipMemcpyAsync(dcp, &one, sizeof one, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din, states_in, sizeof(int32_t) * (size_t)n * c->C, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dev_events, 0, sizeof(unsigned long long), c->stream));
    SimArgs a{};
    a.logtab = c->logtab; a.n = n; a.step = step; a.tmax = max_time; a.cp = dcp; a.in = din; a.out = dout; a.events = dev_events;
    hipError_t le = launch_simulate(a, c->model, c->G, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "simulate launch failed: %s", hipGetErrorString(le));
    unsigned long long ev = 0;
    HIP_TRY(hipMemcpyAsync(states_out, dout, sizeof(int32_t) * (size_t)n * c->C, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&ev, dev_events, sizeof ev, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (events_out) *events_out = (int64_t)ev;
    return EPIPF_OK;
}

int epipf_simulate_path(epipf_ctx* c, int n, const int32_t* states_in, const double* theta, int d, double max_time,
                        uint64_t key, uint32_t filter_index, uint32_t step, int max_events, double* times_out,
                        int32_t* states_out, int32_t* n_events_out, int32_t* final_out) {
    if (!c || !states_in || !theta || !n_events_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 0 || max_events < 0) return fail(EPIPF_EINVAL, "n and max_events must be >= 0");
    if (max_events > 0 && (!times_out || !states_out)) return fail(EPIPF_EINVAL, "NULL path output");
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta needs %d entries", theta_dim(c->model, c->G));
    if (!(max_time >= 0.0)) return fail(EPIPF_EINVAL, "max_time must be >= 0");
    for (int i = 0; i < d; ++i)
        if (!(theta[i] >= 0.0 && theta[i] < INFINITY)) return fail(EPIPF_EINVAL, "theta[%d] must be finite and >= 0", i);
    for (size_t i = 0; i < (size_t)n * c->C; ++i)
        if (states_in[i] < 0) return fail(EPIPF_EINVAL, "states must be non-negative");
    if (n == 0) return EPIPF_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int C = c->C;
    const size_t cap = (size_t)max_events;
    const size_t sb = align256((size_t)n * C * sizeof(int32_t));
    const size_t tb = align256(cap * n * sizeof(double)), xb = align256(cap * n * C * sizeof(int32_t));
    const size_t nb = align256((size_t)n * sizeof(int32_t));
    const size_t need = align256(sizeof(OneChain)) + 2 * sb + tb + xb + nb;
    if (ensure_scratch(c, need)) return EPIPF_ENOMEM;
    char* base = (char*)c->scratch;
    ChainParam* dcp = (ChainParam*)base;
    int32_t* din = (int32_t*)(base + align256(sizeof(OneChain)));
    int32_t* dfin = (int32_t*)((char*)din + sb);
    double* dt = (double*)((char*)dfin + sb);
    int32_t* dx = (int32_t*)((char*)dt + tb);
    int32_t* dnev = (int32_t*)((char*)dx + xb);
    OneChain one;
    memset(&one, 0, sizeof one);
    ChainParam& q = one.q;
    for (int i = 0; i < d; ++i) set_theta(q, c->G > kMaxLaneG ? &one.w : nullptr, i, theta[i]);
    q.k0 = (uint32_t)key; q.k1 = (uint32_t)(key >> 32); q.f = filter_index;
    q.clock_slack = 1.f;
    q.band_slack = 1.f;
    HIP_TRY(hipMemcpyAsync(dcp, &one, sizeof one, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din, states_in, sizeof(int32_t) * (size_t)n * C, hipMemcpyHostToDevice, c->stream));
    SimPathArgs a{};
    a.logtab = c->logtab; a.n = n; a.cap = max_events; a.step = step; a.tmax = max_time; a.cp = dcp; a.in = din;
    a.times = dt; a.states = dx; a.nev = dnev; a.final_state = dfin;
    hipError_t le = launch_simulate_path(a, c->model, c->G, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "simulate_path launch failed: %s", hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(n_events_out, dnev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (final_out)
        HIP_TRY(hipMemcpyAsync(final_out, dfin, sizeof(int32_t) * (size_t)n * C, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> ht;
    std::vector<int32_t> hx;
    if (cap > 0) {
        ht.resize(cap * n);
        hx.resize(cap * n * C);
        HIP_TRY(hipMemcpyAsync(ht.data(), dt, sizeof(double) * cap * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hx.data(), dx, sizeof(int32_t) * cap * n * C, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < n; ++j) {                       // event-major device rows -> one row per trajectory
        const size_t m = std::min<size_t>(cap, (size_t)std::max(n_events_out[j], 0));
        for (size_t e = 0; e < m; ++e) {
            times_out[(size_t)j * cap + e] = ht[e * n + j];
            for (int k = 0; k < C; ++k) states_out[((size_t)j * cap + e) * C + k] = hx[(e * C + k) * n + j];
        }
    }
    trim_scratch(c);
    return EPIPF_OK;
}

int epipf_forecast(epipf_ctx* c, int n_draws, int replicates, int horizon, const double* theta, int d,
                   const int32_t* states, uint64_t key, uint32_t filter_index, uint32_t step, int32_t* rows_out,
                   int64_t* sums_out, uint32_t* hist_out, int bins, int64_t* events_out) {
    if (!c || !theta || !states || !sums_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (n_draws < 0) return fail(EPIPF_EINVAL, "n_draws < 0");
    if (replicates < 1) return fail(EPIPF_EINVAL, "replicates must be >= 1");
    if (horizon < 1) return fail(EPIPF_EINVAL, "horizon must be >= 1");
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta needs %d entries", theta_dim(c->model, c->G));
    if ((int64_t)n_draws * replicates > INT32_MAX)
        return fail(EPIPF_EINVAL, "n_draws * replicates must be <= %d", INT32_MAX);
    const int C = c->C;
    if ((int64_t)horizon * C > INT32_MAX)
        return fail(EPIPF_EINVAL, "horizon * %d compartments must be <= %d", C, INT32_MAX);
    // rows_out: the transpose to the caller's layout runs 64 x 64 tiles on a 2-D grid (launch_forecast_transpose)
    if (rows_out && ((int64_t)n_draws * replicates >= ((int64_t)1 << 30) || ((int64_t)horizon * C + 63) / 64 > 65535))
        return fail(EPIPF_EINVAL, "rows_out needs n_draws * replicates < 2^30 and horizon * %d <= %d", C, 65535 * 64);
    for (size_t i = 0; i < (size_t)n_draws * d; ++i)
        if (!(theta[i] >= 0.0 && theta[i] < INFINITY))
            return fail(EPIPF_EINVAL, "theta[%zu][%zu] must be finite and >= 0", i / d, i % d);
    int64_t largest = 0;
    for (int i = 0; i < n_draws; ++i) {
        int64_t total = 0;
        for (int k = 0; k < C; ++k) {
            if (states[(size_t)i * C + k] < 0) return fail(EPIPF_EINVAL, "states must be non-negative");
            total += states[(size_t)i * C + k];
        }
        largest = std::max(largest, total);
    }
    // a compartment never exceeds its draw's total, which every model conserves: int32 rows, and the histogram's range
    if (largest > INT32_MAX) return fail(EPIPF_EINVAL, "a draw's state total must be <= %d", INT32_MAX);
    if (hist_out && (int64_t)bins <= largest)
        return fail(EPIPF_EINVAL, "bins must be > %lld, the largest state total", (long long)largest);
    const size_t HC = (size_t)horizon * C;
    for (size_t i = 0; i < HC; ++i) sums_out[i] = 0;
    if (events_out) *events_out = 0;
    if (n_draws == 0) {
        if (hist_out) memset(hist_out, 0, sizeof(uint32_t) * HC * (size_t)bins);
        return EPIPF_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const bool wide = c->G > kMaxLaneG;
    const int n = n_draws * replicates;
    const size_t pb = align256(cp_slots(c->G, (size_t)n_draws) * sizeof(ChainParam));
    const size_t sb = align256((size_t)n_draws * C * sizeof(int32_t));
    const size_t ub = align256((HC + 1) * sizeof(unsigned long long));          // sums, then the event count
    const size_t hb = hist_out ? align256(HC * (size_t)bins * sizeof(uint32_t)) : 0;
    const size_t rb = rows_out ? align256(HC * (size_t)n * sizeof(int32_t)) : 0;   // lane-minor, then transposed
    if (ensure_scratch(c, pb + sb + ub + hb + 2 * rb)) return EPIPF_ENOMEM;
    char* base = (char*)c->scratch;
    ChainParam* dcp = (ChainParam*)base;
    int32_t* din = (int32_t*)(base + pb);
    unsigned long long* dsums = (unsigned long long*)((char*)din + sb);
    uint32_t* dhist = hist_out ? (uint32_t*)((char*)dsums + ub) : nullptr;
    int32_t* drows = rows_out ? (int32_t*)((char*)dsums + ub + hb) : nullptr;
    // draw i's parameters; its stream is the single-theta calls' at filter index filter_index + i (wrapping)
    std::vector<ChainParam> hcp(cp_slots(c->G, (size_t)n_draws));
    memset(hcp.data(), 0, hcp.size() * sizeof(ChainParam));
    WideParam* hw = wide ? const_cast<WideParam*>(wide_param(hcp.data(), n_draws, 0)) : nullptr;
    for (int i = 0; i < n_draws; ++i) {
        ChainParam& q = hcp[i];
        for (int k = 0; k < d; ++k) set_theta(q, wide ? hw + i : nullptr, k, theta[(size_t)i * d + k]);
        q.k0 = (uint32_t)key; q.k1 = (uint32_t)(key >> 32); q.f = filter_index + (uint32_t)i;
        q.clock_slack = 1.f;
        q.band_slack = 1.f;
    }
    HIP_TRY(hipMemcpyAsync(dcp, hcp.data(), hcp.size() * sizeof(ChainParam), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din, states, sizeof(int32_t) * (size_t)n_draws * C, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dsums, 0, ub + hb, c->stream));
    ForecastArgs a{};
    a.logtab = c->logtab; a.n = n; a.D = n_draws; a.R = replicates; a.H = horizon; a.bins = bins;
    a.lds_sums = forecast_lds_sums(horizon, C) ? 1 : 0;
    a.step = step; a.cp = dcp; a.in = din; a.rows = drows; a.sums = dsums; a.hist = dhist; a.events = dsums + HC;
    hipError_t le = launch_forecast(a, c->model, c->G, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "forecast launch failed: %s", hipGetErrorString(le));
    std::vector<unsigned long long> hs(HC + 1);
    HIP_TRY(hipMemcpyAsync(hs.data(), dsums, sizeof(unsigned long long) * (HC + 1), hipMemcpyDeviceToHost, c->stream));
    if (hist_out)
        HIP_TRY(hipMemcpyAsync(hist_out, dhist, sizeof(uint32_t) * HC * (size_t)bins, hipMemcpyDeviceToHost, c->stream));
    if (rows_out) {                                     // lane-minor device rows -> [draw][replicate][day][compartment]
        int32_t* dout = (int32_t*)((char*)drows + rb);
        le = launch_forecast_transpose(drows, dout, n, (int)HC, c->stream);
        if (le != hipSuccess) return fail(EPIPF_EHIP, "forecast transpose launch failed: %s", hipGetErrorString(le));
        HIP_TRY(hipMemcpyAsync(rows_out, dout, sizeof(int32_t) * HC * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < HC; ++i) sums_out[i] = (int64_t)hs[i];
    if (events_out) *events_out = (int64_t)hs[HC];
    trim_scratch(c);
    return EPIPF_OK;
}

// Path functionals of epipf_forecast's trajectories: the same checks, parameter blocks and streams.
int epipf_forecast_summary(epipf_ctx* c, int n_draws, int replicates, int horizon, const double* theta, int d,
                           const int32_t* states, uint64_t key, uint32_t filter_index, uint32_t step,
                           int32_t* peak_out, double* peak_time_out, double* extinction_time_out,
                           int32_t* infections_out, int32_t* events_out, int64_t* totals_out,
                           uint32_t* peak_hist_out, uint32_t* infections_hist_out, int bins, uint32_t* peak_day_out,
                           uint32_t* extinct_day_out, uint32_t* extinct_per_draw_out) {
    if (!c || !theta || !states || !totals_out || !peak_day_out || !extinct_day_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (n_draws < 0) return fail(EPIPF_EINVAL, "n_draws < 0");
    if (replicates < 1) return fail(EPIPF_EINVAL, "replicates must be >= 1");
    if (horizon < 1) return fail(EPIPF_EINVAL, "horizon must be >= 1");
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta needs %d entries", theta_dim(c->model, c->G));
    if ((int64_t)n_draws * replicates > INT32_MAX)
        return fail(EPIPF_EINVAL, "n_draws * replicates must be <= %d", INT32_MAX);
    if (2 * (int64_t)horizon + 1 > INT32_MAX) return fail(EPIPF_EINVAL, "2 * horizon + 1 must be <= %d", INT32_MAX);
    const int per_path = (peak_out != nullptr) + (peak_time_out != nullptr) + (extinction_time_out != nullptr) +
                         (infections_out != nullptr) + (events_out != nullptr);
    if (per_path != 0 && per_path != 5)
        return fail(EPIPF_EINVAL, "the five per-path outputs must be all NULL or all non-NULL");
    if ((peak_hist_out != nullptr) != (infections_hist_out != nullptr))
        return fail(EPIPF_EINVAL, "the two value histograms must be both NULL or both non-NULL");
    const bool hist = peak_hist_out != nullptr;
    const int C = c->C;
    for (size_t i = 0; i < (size_t)n_draws * d; ++i)
        if (!(theta[i] >= 0.0 && theta[i] < INFINITY))
            return fail(EPIPF_EINVAL, "theta[%zu][%zu] must be finite and >= 0", i / d, i % d);
    int64_t largest = 0;
    for (int i = 0; i < n_draws; ++i) {
        int64_t total = 0;
        for (int k = 0; k < C; ++k) {
            if (states[(size_t)i * C + k] < 0) return fail(EPIPF_EINVAL, "states must be non-negative");
            total += states[(size_t)i * C + k];
        }
        largest = std::max(largest, total);
    }
    // the peak and the infections never exceed a draw's total, which every model conserves: int32, and the histograms' range
    if (largest > INT32_MAX) return fail(EPIPF_EINVAL, "a draw's state total must be <= %d", INT32_MAX);
    if (hist && (int64_t)bins <= largest)
        return fail(EPIPF_EINVAL, "bins must be > %lld, the largest state total", (long long)largest);
    const size_t H = (size_t)horizon;
    for (int i = 0; i < 4; ++i) totals_out[i] = 0;
    if (n_draws == 0) {
        memset(peak_day_out, 0, sizeof(uint32_t) * H);
        memset(extinct_day_out, 0, sizeof(uint32_t) * (H + 1));
        if (hist) {
            memset(peak_hist_out, 0, sizeof(uint32_t) * (size_t)bins);
            memset(infections_hist_out, 0, sizeof(uint32_t) * (size_t)bins);
        }
        return EPIPF_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const bool wide = c->G > kMaxLaneG;
    const int n = n_draws * replicates;
    const size_t pb = align256(cp_slots(c->G, (size_t)n_draws) * sizeof(ChainParam));
    const size_t sb = align256((size_t)n_draws * C * sizeof(int32_t));
    // the reductions, zeroed together: totals [4] u64, then uint32 peak_day [H], extinct_day [H + 1],
    // extinct_per_draw [D], peak_hist [bins], infections_hist [bins]
    const size_t nb = hist ? (size_t)bins : 0;
    const size_t n32 = 2 * H + 1 + (size_t)n_draws + 2 * nb;
    const size_t ub = align256(4 * sizeof(unsigned long long) + n32 * sizeof(uint32_t));
    const size_t fb = per_path ? align256((size_t)n * sizeof(double)) : 0;     // per path: two f64, then three int32
    const size_t ib = per_path ? align256((size_t)n * sizeof(int32_t)) : 0;
    if (ensure_scratch(c, pb + sb + ub + 2 * fb + 3 * ib)) return EPIPF_ENOMEM;
    char* base = (char*)c->scratch;
    ChainParam* dcp = (ChainParam*)base;
    int32_t* din = (int32_t*)(base + pb);
    unsigned long long* dtot = (unsigned long long*)(base + pb + sb);
    uint32_t* dpday = (uint32_t*)(dtot + 4);
    uint32_t* deday = dpday + H;
    uint32_t* ddraw = deday + H + 1;
    uint32_t* dphist = ddraw + n_draws;
    uint32_t* dihist = dphist + nb;
    double* dptime = (double*)(base + pb + sb + ub);
    double* detime = (double*)((char*)dptime + fb);
    int32_t* dpeak = (int32_t*)((char*)detime + fb);
    int32_t* dinf = (int32_t*)((char*)dpeak + ib);
    int32_t* dnev = (int32_t*)((char*)dinf + ib);
    // draw i's parameters; its stream is the single-theta calls' at filter index filter_index + i (wrapping)
    std::vector<ChainParam> hcp(cp_slots(c->G, (size_t)n_draws));
    memset(hcp.data(), 0, hcp.size() * sizeof(ChainParam));
    WideParam* hw = wide ? const_cast<WideParam*>(wide_param(hcp.data(), n_draws, 0)) : nullptr;
    for (int i = 0; i < n_draws; ++i) {
        ChainParam& q = hcp[i];
        for (int k = 0; k < d; ++k) set_theta(q, wide ? hw + i : nullptr, k, theta[(size_t)i * d + k]);
        q.k0 = (uint32_t)key; q.k1 = (uint32_t)(key >> 32); q.f = filter_index + (uint32_t)i;
        q.clock_slack = 1.f;
        q.band_slack = 1.f;
    }
    HIP_TRY(hipMemcpyAsync(dcp, hcp.data(), hcp.size() * sizeof(ChainParam), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din, states, sizeof(int32_t) * (size_t)n_draws * C, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dtot, 0, ub, c->stream));
    long long lds_limit = -1;                            // bytes; lowers kForecastSummaryLdsDays (for tests)
    if (const char* e = getenv("EPIPF_FORECAST_SUMMARY_LDS")) lds_limit = std::max(0ll, atoll(e));
    ForecastSummaryArgs a{};
    a.logtab = c->logtab; a.n = n; a.D = n_draws; a.R = replicates; a.H = horizon; a.bins = bins;
    a.lds_days = forecast_summary_lds_days(horizon, lds_limit) ? 1 : 0;
    a.step = step; a.cp = dcp; a.in = din;
    if (per_path) { a.peak = dpeak; a.peak_time = dptime; a.extinction_time = detime; a.infections = dinf; a.events = dnev; }
    a.totals = dtot; a.peak_day = dpday; a.extinct_day = deday;
    if (hist) { a.peak_hist = dphist; a.infections_hist = dihist; }
    a.extinct_per_draw = extinct_per_draw_out ? ddraw : nullptr;
    hipError_t le = launch_forecast_summary(a, c->model, c->G, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "forecast summary launch failed: %s", hipGetErrorString(le));
    unsigned long long ht[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(ht, dtot, sizeof ht, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(peak_day_out, dpday, sizeof(uint32_t) * H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(extinct_day_out, deday, sizeof(uint32_t) * (H + 1), hipMemcpyDeviceToHost, c->stream));
    if (extinct_per_draw_out)
        HIP_TRY(hipMemcpyAsync(extinct_per_draw_out, ddraw, sizeof(uint32_t) * (size_t)n_draws, hipMemcpyDeviceToHost, c->stream));
    if (hist) {
        HIP_TRY(hipMemcpyAsync(peak_hist_out, dphist, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(infections_hist_out, dihist, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, c->stream));
    }
    if (per_path) {
        HIP_TRY(hipMemcpyAsync(peak_out, dpeak, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(peak_time_out, dptime, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(extinction_time_out, detime, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(infections_out, dinf, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(events_out, dnev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; ++i) totals_out[i] = (int64_t)ht[i];
    trim_scratch(c);
    return EPIPF_OK;
}

// ------------------------------------------------------------------------------- particle smoother
// One chain's histogram above this is refused (as epipf.forecast refuses its own); the chains of a call share at most
// kSmoothScratch of histogram and global multiplicity rows, in slices (EPIPF_SMOOTH_SCRATCH_MB overrides, for tests).
constexpr size_t kSmoothHistLimit = (size_t)256 << 20;
constexpr size_t kSmoothScratch = (size_t)4 << 30;

constexpr int kSmoothNoLag = -1;

// The smoother over n chains of [T][N][C] histories: the context's own (up_hidden == NULL: its strides and the last
// run's status), the caller's host arrays, uploaded to scratch, or (flows: up_hidden == NULL, C = F) the true flows of
// the context's own history, formed on the device into scratch with its ancestry and status.  lag >= 0 is the fixed-lag pass (§16.1, `kind` is
// EPIPF_SMOOTH_SMOOTHING): one workgroup per (chain, day), the days of a chain sliced too when its global rows alone
// exceed the budget; lag >= T - 1 is the smoother itself and runs as it.
static int smooth_run(epipf_ctx* c, int n, int T, int N, int C, const int32_t* up_hidden, const int32_t* up_ancestry,
                      int lineage, int kind, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                      int32_t* quant_out, int32_t* lineages_out, bool flows = false) {
    if (!sums_out || !lineages_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (lineage != EPIPF_LINEAGE_REFERENCE && lineage != EPIPF_LINEAGE_GENEALOGY)
        return fail(EPIPF_EINVAL, "unknown lineage %d", lineage);
    if (kind != EPIPF_SMOOTH_SMOOTHING && kind != EPIPF_SMOOTH_PREDICTIVE) return fail(EPIPF_EINVAL, "unknown kind %d", kind);
    if (n_q < 0 || (n_q > 0 && !q)) return fail(EPIPF_EINVAL, "n_q=%d needs q", n_q);
    if (n_q > 0 && (bins < 1 || !quant_out)) return fail(EPIPF_EINVAL, "quantiles need bins >= 1 and quant_out");
    for (int i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(EPIPF_EINVAL, "q[%d] must lie in [0, 1]", i);
    if (C > kSmoothMaxC) return fail(EPIPF_EINVAL, "at most %d compartments, got %d", kSmoothMaxC, C);
    if (N > kSmoothMaxN) return fail(EPIPF_EINVAL, "at most %d particles, got %d", kSmoothMaxN, N);
    const size_t TC = (size_t)T * C;
    const size_t hb1 = n_q > 0 ? TC * (size_t)bins * sizeof(uint32_t) : 0;   // one chain's histogram
    if (hb1 > kSmoothHistLimit)
        return fail(EPIPF_EINVAL, "the quantile histogram needs %zu bytes (> %zu): call with no quantiles and reduce the "
                    "history instead", hb1, kSmoothHistLimit);
    const bool predictive = kind == EPIPF_SMOOTH_PREDICTIVE;
    bool lds_rows = N <= kSmoothLdsMaxN;
    if (const char* e = getenv("EPIPF_SMOOTH_LDS")) lds_rows = lds_rows && atoi(e) != 0;
    const bool lagged = lag >= 0 && lag < T - 1;
    const size_t rb1 = (predictive || lds_rows) ? 0 : 2 * sizeof(uint32_t) * (size_t)N;   // one workgroup's global rows
    size_t budget = kSmoothScratch;
    if (const char* e = getenv("EPIPF_SMOOTH_SCRATCH_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    // days per launch of the fixed-lag pass (a workgroup each, with its own global rows): all T, or what the budget holds
    // beside one chain's histogram, at least one
    int days = T;
    if (lagged) {
        if (rb1 > 0 && hb1 + (size_t)T * rb1 > budget)
            days = (int)std::max<size_t>(1, std::min<size_t>((size_t)T, (budget > hb1 ? budget - hb1 : 0) / rb1));
        days = std::min(days, kSmoothLagMaxBlocks);
    }
    const size_t mb1 = lagged ? (size_t)days * rb1 : rb1;   // one chain's global rows
    // chains per slice: what the budget holds, at least one (one chain's histogram is within kSmoothHistLimit)
    int slice = n;
    if (hb1 + mb1 > 0) slice = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, budget / (hb1 + mb1)));
    if (lagged) slice = std::min(slice, std::max(1, kSmoothLagMaxBlocks / days));
    HIP_TRY(hipSetDevice(c->device));
    const size_t ob_s = align256((size_t)n * TC * sizeof(unsigned long long));
    const size_t ob_l = align256((size_t)n * T * sizeof(int32_t));
    const size_t ob_q = n_q > 0 ? align256((size_t)n * n_q * TC * sizeof(int32_t)) : 0;
    const size_t ob_r = n_q > 0 ? align256((size_t)n_q * sizeof(uint32_t)) : 0;
    const size_t sb_h = align256((size_t)slice * hb1), sb_m = align256((size_t)slice * mb1);
    const size_t ub_h = (up_hidden || flows) ? align256((size_t)n * T * N * C * sizeof(int32_t)) : 0;
    const size_t ub_a = up_hidden ? align256((size_t)n * T * N * sizeof(int32_t)) : 0;
    if (ensure_scratch(c, ob_s + ob_l + ob_q + ob_r + sb_h + sb_m + ub_h + ub_a)) return EPIPF_ENOMEM;
    char* p = (char*)c->scratch;
    unsigned long long* dsums = (unsigned long long*)p; p += ob_s;
    int32_t* dlin = (int32_t*)p; p += ob_l;
    int32_t* dquant = (int32_t*)p; p += ob_q;
    uint32_t* dranks = (uint32_t*)p; p += ob_r;
    uint32_t* dhist = (uint32_t*)p; p += sb_h;
    uint32_t* drows = (uint32_t*)p; p += sb_m;
    int32_t* dhid = (int32_t*)p; p += ub_h;
    int32_t* danc = (int32_t*)p;
    HIP_TRY(hipMemsetAsync(dsums, 0, ob_s + ob_l + ob_q, c->stream));
    std::vector<uint32_t> ranks((size_t)n_q);
    uint32_t max_rank = 0;
    for (int i = 0; i < n_q; ++i) {                      // numpy's inverted_cdf rule, q N in float64
        ranks[i] = (uint32_t)std::max(std::ceil(q[i] * (double)N), 1.0);
        max_rank = std::max(max_rank, ranks[i]);
    }
    if (n_q > 0) HIP_TRY(hipMemcpyAsync(dranks, ranks.data(), sizeof(uint32_t) * n_q, hipMemcpyHostToDevice, c->stream));
    SmoothArgs a{};
    a.T = T; a.N = N; a.C = C; a.shift = lineage == EPIPF_LINEAGE_GENEALOGY ? 1 : 0; a.predictive = predictive ? 1 : 0;
    a.bins = bins; a.sums = dsums; a.lineages = dlin;
    if (up_hidden) {
        HIP_TRY(hipMemcpyAsync(dhid, up_hidden, sizeof(int32_t) * (size_t)n * T * N * C, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(danc, up_ancestry, sizeof(int32_t) * (size_t)n * T * N, hipMemcpyHostToDevice, c->stream));
        a.hidden = dhid; a.ancestry = danc; a.status = nullptr;
        a.hist_stride = (size_t)T * N * C; a.anc_stride = (size_t)T * N;
    } else if (flows) {
        IncidenceFlowArgs fa{};
        fa.n = n; fa.T = T; fa.N = N; fa.hist_stride = c->hist_stride; fa.anc_stride = c->anc_stride;
        fa.hidden = c->hidden; fa.ancestry = c->ancestry; fa.flow = dhid;
        const hipError_t fe = launch_incidence_flows(fa, c->model, c->stream);
        if (fe != hipSuccess) return fail(EPIPF_EHIP, "flow launch failed: %s", hipGetErrorString(fe));
        a.hidden = dhid; a.ancestry = c->ancestry; a.status = c->status;
        a.hist_stride = (size_t)T * N * C; a.anc_stride = c->anc_stride;
    } else {
        a.hidden = c->hidden; a.ancestry = c->ancestry; a.status = c->status;
        a.hist_stride = c->hist_stride; a.anc_stride = c->anc_stride;
    }
    for (int c0 = 0; c0 < n; c0 += slice) {
        const int k = std::min(slice, n - c0);
        a.n = k; a.chain0 = c0;
        a.mrows = mb1 ? drows : nullptr;
        a.hist = hb1 ? dhist : nullptr;
        if (hb1) HIP_TRY(hipMemsetAsync(dhist, 0, (size_t)k * hb1, c->stream));
        hipError_t le = hipSuccess;
        if (lagged) {
            SmoothLagArgs la{};
            la.n = k; la.chain0 = c0; la.T = T; la.N = N; la.C = C; la.shift = a.shift; la.lag = lag; la.bins = bins;
            la.hist_stride = a.hist_stride; la.anc_stride = a.anc_stride; la.hidden = a.hidden; la.ancestry = a.ancestry;
            la.status = a.status; la.mrows = a.mrows; la.sums = dsums; la.lineages = dlin; la.hist = a.hist;
            for (int d0 = 0; d0 < T && le == hipSuccess; d0 += days) {
                la.day0 = d0; la.days = std::min(days, T - d0);
                le = launch_smooth_lag(la, c->stream);
            }
        } else {
            le = launch_smooth(a, c->stream);
        }
        if (le != hipSuccess) return fail(EPIPF_EHIP, "smooth launch failed: %s", hipGetErrorString(le));
        if (n_q > 0) {
            SmoothQuantArgs qa{};
            qa.n = k; qa.chain0 = c0; qa.T = T; qa.C = C; qa.bins = bins; qa.n_q = n_q; qa.max_rank = max_rank;
            qa.status = a.status; qa.hist = dhist; qa.ranks = dranks; qa.quant = dquant;
            le = launch_smooth_quantiles(qa, c->stream);
            if (le != hipSuccess) return fail(EPIPF_EHIP, "smooth quantile launch failed: %s", hipGetErrorString(le));
        }
    }
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "sums are copied out as they are");
    HIP_TRY(hipMemcpyAsync(sums_out, dsums, sizeof(int64_t) * (size_t)n * TC, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(lineages_out, dlin, sizeof(int32_t) * (size_t)n * T, hipMemcpyDeviceToHost, c->stream));
    if (n_q > 0)
        HIP_TRY(hipMemcpyAsync(quant_out, dquant, sizeof(int32_t) * (size_t)n * n_q * TC, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    trim_scratch(c);
    return EPIPF_OK;
}

// epipf_smooth / epipf_smooth_lag: the last run's chains, resident on the device.
static int smooth_resident(epipf_ctx* c, int n_chains, int lineage, int kind, int lag, const double* q, int n_q, int bins,
                           int64_t* sums_out, int32_t* quant_out, int32_t* lineages_out) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (!c->have_run) return fail(EPIPF_ESTATE, "no filter has run on this context");
    if (n_chains < 1 || n_chains > c->last_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->last_chains);
    return smooth_run(c, n_chains, c->last_T, c->N, c->C, nullptr, nullptr, lineage, kind, lag, q, n_q, bins, sums_out,
                      quant_out, lineages_out);
}

// epipf_smooth_history / epipf_smooth_lag_history: the caller's host arrays.
static int smooth_uploaded(epipf_ctx* c, int n, int T, int N, int C, const int32_t* hidden, const int32_t* ancestry,
                           int lineage, int kind, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                           int32_t* quant_out, int32_t* lineages_out) {
    if (!c || !hidden || !ancestry) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 1 || T < 1 || N < 1 || C < 1) return fail(EPIPF_EINVAL, "n, T, N, C must be >= 1");
    if ((double)n * T * N * C > (double)((size_t)1 << 40)) return fail(EPIPF_EINVAL, "history too large");
    for (size_t i = 0; i < (size_t)n * T * N * C; ++i)
        if (hidden[i] < 0) return fail(EPIPF_EINVAL, "counts must be non-negative");
    for (size_t i = 0; i < (size_t)n * T * N; ++i)
        if (ancestry[i] < 0 || ancestry[i] >= N) return fail(EPIPF_EINVAL, "ancestors must lie in [0, N)");
    return smooth_run(c, n, T, N, C, hidden, ancestry, lineage, kind, lag, q, n_q, bins, sums_out, quant_out, lineages_out);
}

int epipf_smooth(epipf_ctx* c, int n_chains, int lineage, int kind, const double* q, int n_q, int bins,
                 int64_t* sums_out, int32_t* quant_out, int32_t* lineages_out) {
    return smooth_resident(c, n_chains, lineage, kind, kSmoothNoLag, q, n_q, bins, sums_out, quant_out, lineages_out);
}

int epipf_smooth_history(epipf_ctx* c, int n, int T, int N, int C, const int32_t* hidden, const int32_t* ancestry,
                         int lineage, int kind, const double* q, int n_q, int bins, int64_t* sums_out,
                         int32_t* quant_out, int32_t* lineages_out) {
    return smooth_uploaded(c, n, T, N, C, hidden, ancestry, lineage, kind, kSmoothNoLag, q, n_q, bins, sums_out, quant_out,
                           lineages_out);
}

// The fixed-lag smoother: the same checks, and the lag's.
int epipf_smooth_lag(epipf_ctx* c, int n_chains, int lineage, int lag, const double* q, int n_q, int bins,
                     int64_t* sums_out, int32_t* quant_out, int32_t* lineages_out) {
    if (lag < 0) return fail(EPIPF_EINVAL, "lag=%d must be >= 0", lag);
    return smooth_resident(c, n_chains, lineage, EPIPF_SMOOTH_SMOOTHING, lag, q, n_q, bins, sums_out, quant_out,
                           lineages_out);
}

int epipf_smooth_lag_history(epipf_ctx* c, int n, int T, int N, int C, const int32_t* hidden, const int32_t* ancestry,
                             int lineage, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                             int32_t* quant_out, int32_t* lineages_out) {
    if (lag < 0) return fail(EPIPF_EINVAL, "lag=%d must be >= 0", lag);
    return smooth_uploaded(c, n, T, N, C, hidden, ancestry, lineage, EPIPF_SMOOTH_SMOOTHING, lag, q, n_q, bins, sums_out,
                           quant_out, lineages_out);
}

// Iterated filtering: M passes of the filter with theta per particle, all enqueued at once.
// epipf_if2 (SIR, SEIR) and epipf_iterated_filtering_subgroups (the subgroup models at G <= kMaxLaneG) are this
// function behind their own model checks; only the launcher differs.
static int if2_impl(epipf_ctx* c, bool subgroups, int n_searches, int iterations, double* swarm_inout, int d,
                    const double* half_widths, int obs_model, const double* probs, const uint64_t* keys,
                    const uint32_t* filter_index0, double* log_zetas_out, double* mean_out,
                    int32_t* iterations_done_out, int32_t* status_out) {
    if (!c->have_Y) return fail(EPIPF_ESTATE, "epipf_set_observations was not called");
    if (!c->have_pop) return fail(EPIPF_ESTATE, "epipf_set_population was not called");
    const int S = n_searches, M = iterations, N = c->N, T = c->T;
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta has %d entries per particle, model needs %d", d, theta_dim(c->model, c->G));
    if (S < 1 || S > c->max_chains) return fail(EPIPF_EINVAL, "n_searches=%d outside [1, max_chains=%d]", S, c->max_chains);
    if (M < 1) return fail(EPIPF_EINVAL, "iterations=%d must be >= 1", M);
    if (obs_model != EPIPF_OBS_BINOMIAL && obs_model != EPIPF_OBS_NORMAL) return fail(EPIPF_EINVAL, "bad obs_model %d", obs_model);
    if (const int e = check_swarm(half_widths, (size_t)M, swarm_inout, (size_t)S, N, d)) return e;
    for (int s = 0; s < S; ++s) {
        ChainParam& q = c->h_cp[s];
        memset(&q, 0, sizeof q);                         // theta is the particles' own (the swarm)
        set_chain_stream(c, q, probs[s], keys[s], filter_index0[s]);
        q.chosen = -1;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->walk_valid = false;                               // the history is this call's from here on
    c->inc_valid = false;
    // scratch: swarm [2][max_chains][d][N] | start [max_chains][d][N] | log_zeta [M][max_chains][T] | mean [S][M][d] | done [S]
    const size_t comp = (size_t)d * N, mc = (size_t)c->max_chains;
    const size_t b_swarm = align256(sizeof(double) * 2 * mc * comp), b_start = align256(sizeof(double) * mc * comp);
    const size_t b_lz = align256(sizeof(double) * (size_t)M * mc * T), b_mean = align256(sizeof(double) * (size_t)S * M * d);
    const size_t b_done = align256(sizeof(int32_t) * (size_t)S);
    if (ensure_scratch(c, b_swarm + b_start + b_lz + b_mean + b_done)) return EPIPF_ENOMEM;
    char* base = (char*)c->scratch;
    double* d_swarm = (double*)base;
    double* d_start = (double*)(base + b_swarm);
    double* d_lz = (double*)(base + b_swarm + b_start);
    double* d_mean = (double*)(base + b_swarm + b_start + b_lz);
    int32_t* d_done = (int32_t*)(base + b_swarm + b_start + b_lz + b_mean);
    std::vector<double> soa((size_t)S * comp);            // [S][N][d] -> [S][d][N]
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < d; ++k) soa[((size_t)s * d + k) * N + j] = swarm_inout[((size_t)s * N + j) * d + k];
    HIP_TRY(hipMemcpyAsync(c->cp, c->h_cp, sizeof(ChainParam) * S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_start, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_lz, 0xFF, b_lz + b_mean, c->stream));     // rows never written read as NaN
    HIP_TRY(hipMemsetAsync(d_done, 0, b_done, c->stream));
    // the device counters of this call alone: cleared here and again once harvested, so that neither an earlier run's
    // counts are reported as this call's nor this call's as the next epipf_run's
    const size_t b_counters = sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride;
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));

    If2Args a{};
    StepArgs& s = a.s;
    one_lane_step_args(c, T, s);
    s.log_zeta = d_lz;                                   // [M][max_chains][T], a row block per iteration
    a.d = d; a.M = M; a.swarm = d_swarm; a.start = d_start; a.mean = d_mean; a.done = d_done;

    FilterStreams fs{};
    if (const int e = fork_streams(c, std::min(c->n_streams, S), fs)) return e;
    hipError_t le = subgroups ? launch_if2_sub(a, c->model, c->G, obs_model, S, half_widths, fs)
                              : launch_if2(a, c->model, obs_model, S, half_widths, fs);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
    std::vector<double> lz((size_t)M * mc * T), mean((size_t)S * M * d);
    HIP_TRY(hipMemcpyAsync(soa.data(), d_start, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(lz.data(), d_lz, sizeof(double) * lz.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(mean.data(), d_mean, sizeof(double) * mean.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(iterations_done_out, d_done, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->status, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_counters, c->counters, b_counters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    harvest_counters(c, s.count_events != 0, false);
    int64_t passes = 0;
    for (int q = 0; q < S; ++q) {
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < d; ++k) swarm_inout[((size_t)q * N + j) * d + k] = soa[((size_t)q * d + k) * N + j];
        const int done = std::min(std::max(iterations_done_out[q], 0), M);
        passes += std::min(done + 1, M);
        for (int m = 0; m < M; ++m) {                    // an iteration that did not complete reports NaN
            for (int k = 0; k < d; ++k)
                mean_out[((size_t)q * M + m) * d + k] = m < done ? mean[((size_t)q * M + m) * d + k] : NAN;
            if (!log_zetas_out) continue;
            for (int p = 0; p < T; ++p)
                log_zetas_out[((size_t)q * M + m) * T + p] = m < done ? lz[((size_t)m * mc + q) * T + p] : NAN;
        }
    }
    c->stats.particle_steps += passes * N * T;
    c->stats.filters += passes;
    c->stats.last_lanes = 1;
    c->stats.last_lane_events = 1;
    c->stats.last_fused = 0;
    c->last_chains = S;
    c->last_T = T;
    c->have_run = true;
    trim_scratch(c);
    return EPIPF_OK;
}

int epipf_if2(epipf_ctx* c, int n_searches, int iterations, double* swarm_inout, int d, const double* half_widths,
              int obs_model, const double* probs, const uint64_t* keys, const uint32_t* filter_index0,
              double* log_zetas_out, double* mean_out, int32_t* iterations_done_out, int32_t* status_out) {
    if (!c || !swarm_inout || !half_widths || !probs || !keys || !filter_index0 || !mean_out || !iterations_done_out ||
        !status_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (c->model != EPIPF_SIR && c->model != EPIPF_SEIR)
        return fail(EPIPF_EINVAL, "iterated filtering covers the SIR and SEIR models; the subgroup models are out of its scope "
                                  "(epipf_iterated_filtering_subgroups runs them at G <= %d)", kMaxLaneG);
    return if2_impl(c, false, n_searches, iterations, swarm_inout, d, half_widths, obs_model, probs, keys, filter_index0,
                    log_zetas_out, mean_out, iterations_done_out, status_out);
}

// The subgroup models' entry point: theta = beta[G][G] row-major then gamma, d = G*G + 1, G <= 4.
// G = 5..8 read their rates through WideParam by wave-uniform address, which a per-particle theta is not.
int epipf_iterated_filtering_subgroups(epipf_ctx* c, int n_searches, int iterations, double* swarm_inout, int d,
                                       const double* half_widths, int obs_model, const double* probs,
                                       const uint64_t* keys, const uint32_t* filter_index0, double* log_zetas_out,
                                       double* mean_out, int32_t* iterations_done_out, int32_t* status_out) {
    if (!c || !swarm_inout || !half_widths || !probs || !keys || !filter_index0 || !mean_out || !iterations_done_out ||
        !status_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (c->model != EPIPF_SIR_SUBGROUPS && c->model != EPIPF_SIR_SUBGROUPS2)
        return fail(EPIPF_EINVAL, "epipf_iterated_filtering_subgroups covers the subgroup models; epipf_if2 runs SIR and SEIR");
    if (c->G < 2 || c->G > kMaxLaneG)
        return fail(EPIPF_EINVAL, "iterated filtering of the subgroup models needs 2 <= G <= %d groups, this context has %d",
                    kMaxLaneG, c->G);
    return if2_impl(c, true, n_searches, iterations, swarm_inout, d, half_widths, obs_model, probs, keys, filter_index0,
                    log_zetas_out, mean_out, iterations_done_out, status_out);
}

// theta_hist [S][T][d][N] of the random-walk filters (epipf_walk_filter, epipf_incidence_walk): grown when a call needs more.
static int ensure_walk_theta(epipf_ctx* c, int S, int T, int d, int N) {
    const size_t need = sizeof(double) * (size_t)S * T * d * N;
    if (need > c->walk_bytes) {
        if (c->walk_theta) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->walk_theta); }
        c->walk_theta = nullptr;
        c->walk_bytes = 0;
        if (hipMalloc((void**)&c->walk_theta, need) != hipSuccess) {
            c->walk_theta = nullptr;
            (void)hipGetLastError();
            return fail(EPIPF_ENOMEM, "the parameter history needs %zu bytes (%d chains x %d days x %d x %d doubles): hipMalloc failed",
                        need, S, T, d, N);
        }
        c->walk_bytes = need;
    }
    return 0;
}

// ------------------------------------------------------------------------ time-varying rates
// The random-walk filter: epipf_if2's pass at one iteration with a half-width vector per chain, every day's swarm kept
// in theta_hist.  hidden, ancestry, status and log_zeta are the context's own, so epipf_copy_history, epipf_path_sample
// and epipf_smooth see the pass afterwards.
int epipf_walk_filter(epipf_ctx* c, int n_chains, const double* swarm_in, int d, const double* half_widths, int obs_model,
                      const double* probs, const uint64_t* keys, const uint32_t* filter_index, double* log_zetas_out,
                      int32_t* status_out) {
    if (!c || !swarm_in || !half_widths || !probs || !keys || !filter_index || !log_zetas_out || !status_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (c->model != EPIPF_SIR && c->model != EPIPF_SEIR)
        return fail(EPIPF_EINVAL, "the random-walk filter covers the SIR and SEIR models; the subgroup models are out of its scope");
    if (!c->have_Y) return fail(EPIPF_ESTATE, "epipf_set_observations was not called");
    if (!c->have_pop) return fail(EPIPF_ESTATE, "epipf_set_population was not called");
    const int S = n_chains, N = c->N, T = c->T;
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta has %d entries per particle, model needs %d", d, theta_dim(c->model, c->G));
    if (S < 1 || S > c->max_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, max_chains=%d]", S, c->max_chains);
    if (obs_model != EPIPF_OBS_BINOMIAL && obs_model != EPIPF_OBS_NORMAL) return fail(EPIPF_EINVAL, "bad obs_model %d", obs_model);
    if (const int e = check_swarm(half_widths, (size_t)S, swarm_in, (size_t)S, N, d)) return e;
    for (int s = 0; s < S; ++s) {
        ChainParam& q = c->h_cp[s];
        memset(&q, 0, sizeof q);                         // theta is the particles' own
        set_chain_stream(c, q, probs[s], keys[s], filter_index[s]);
        q.chosen = -1;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->walk_valid = false;
    c->inc_valid = false;
    const size_t comp = (size_t)d * N, stride = (size_t)T * comp;
    if (const int e = ensure_walk_theta(c, S, T, d, N)) return e;
    // scratch: start [S][d][N] | hw [S][d]
    const size_t b_start = align256(sizeof(double) * (size_t)S * comp), b_hw = align256(sizeof(double) * (size_t)S * d);
    if (ensure_scratch(c, b_start + b_hw)) return EPIPF_ENOMEM;
    double* d_start = (double*)c->scratch;
    double* d_hw = (double*)((char*)c->scratch + b_start);
    std::vector<double> soa((size_t)S * comp);            // [S][N][d] -> [S][d][N]
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < d; ++k) soa[((size_t)s * d + k) * N + j] = swarm_in[((size_t)s * N + j) * d + k];
    HIP_TRY(hipMemcpyAsync(c->cp, c->h_cp, sizeof(ChainParam) * S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_start, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_hw, half_widths, sizeof(double) * (size_t)S * d, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->log_zeta, 0xFF, sizeof(double) * (size_t)S * T, c->stream));   // rows never written read as NaN
    const size_t b_counters = sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride;
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));

    WalkArgs a{};
    StepArgs& s = a.s;
    one_lane_step_args(c, T, s);
    a.d = d; a.hw = d_hw; a.start = d_start; a.hist = c->walk_theta; a.chain_stride = stride;

    FilterStreams fs{};
    if (const int e = fork_streams(c, std::min(c->n_streams, S), fs)) return e;
    const hipError_t le = launch_walk(a, c->model, obs_model, S, fs);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(log_zetas_out, c->log_zeta, sizeof(double) * (size_t)S * T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->status, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_counters, c->counters, b_counters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    harvest_counters(c, s.count_events != 0, false);
    // a chain that died at step p wrote -inf there and nothing after: its later days are -inf as well
    for (int q = 0; q < S; ++q)
        if (status_out[q] == EPIPF_STATUS_DEGENERATE)
            for (int p = 0; p < T; ++p)
                if (std::isnan(log_zetas_out[(size_t)q * T + p])) log_zetas_out[(size_t)q * T + p] = -INFINITY;
    c->stats.particle_steps += (int64_t)S * N * T;
    c->stats.filters += S;
    c->stats.last_lanes = 1;
    c->stats.last_lane_events = 1;
    c->stats.last_fused = 0;
    c->last_chains = S;
    c->last_T = T;
    c->have_run = true;
    c->walk_valid = true;
    trim_scratch(c);
    return EPIPF_OK;
}

// ------------------------------------------------------------------------ incidence observations
// What epipf_run_incidence and epipf_incidence_walk share.  incidence_rows: the reports checked and padded to rows
// [D + 2][F] (rows 0 and D + 1 all NaN) with the reported-column masks rep [D + 2].  incidence_probs: a chain's probs.
// ensure_incidence_counts / ensure_incidence_acc: the device buffers of the reports and of the accumulator
// int32 [2][S][F][N], grown when a call needs more, the latter within its budget.
static int incidence_rows(const double* counts, int D, int F, int obs_model, std::vector<double>& rows,
                          std::vector<uint8_t>& rep) {
    const int T = D + 2;
    rows.assign((size_t)T * F, NAN);
    rep.assign((size_t)T, 0);
    for (size_t i = 0; i < (size_t)D * F; ++i) {
        const double y = counts[i];
        if (std::isnan(y)) continue;                                     // not reported
        if (std::isinf(y) || y < 0.0)
            return fail(EPIPF_EINVAL, "counts[%zu][%zu]=%g: a report must be finite and >= 0 (NaN: not reported)", i / F, i % F, y);
        if (obs_model != EPIPF_OBS_NORMAL && y != std::floor(y))
            return fail(EPIPF_EINVAL, "counts[%zu][%zu]=%g: the %s model needs integer reports", i / F, i % F, y,
                        obs_model == EPIPF_OBS_NEGBIN ? "negative-binomial" : "binomial");
        rows[(size_t)F + i] = y;
        rep[1 + i / F] |= (uint8_t)(1u << (i % F));
    }
    return 0;
}

static int incidence_probs(int ch, double pr, int obs_model) {
    if (!(pr >= 0.0 && pr < INFINITY && (obs_model == EPIPF_OBS_NORMAL || pr <= 1.0)))
        return fail(EPIPF_EINVAL, "probs[%d]=%g: %s", ch, pr,
                    obs_model == EPIPF_OBS_NORMAL ? "the noise ratio must be finite and >= 0"
                                                  : "the reporting probability must lie in [0, 1]");
    return 0;
}

static int ensure_incidence_counts(epipf_ctx* c, size_t n) {
    if (n > c->inc_counts_n) {
        if (c->inc_counts) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->inc_counts); }
        c->inc_counts = nullptr;
        c->inc_counts_n = 0;
        if (dalloc(&c->inc_counts, n)) return EPIPF_ENOMEM;
        c->inc_counts_n = n;
    }
    return 0;
}

static int ensure_incidence_acc(epipf_ctx* c, int S, int F, int N) {
    const size_t need = 2 * sizeof(int32_t) * (size_t)S * F * N;
    if (need > c->inc_acc_bytes) {
        if (c->inc_acc_limit && need > c->inc_acc_limit)
            return fail(EPIPF_ENOMEM, "the accumulator needs %zu bytes (2 x %d chains x %d columns x %d int32): over the budget of %zu bytes",
                        need, S, F, N, c->inc_acc_limit);
        if (c->inc_acc) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->inc_acc); }
        c->inc_acc = nullptr;
        c->inc_acc_bytes = 0;
        if (hipMalloc((void**)&c->inc_acc, need) != hipSuccess) {
            c->inc_acc = nullptr;
            (void)hipGetLastError();
            return fail(EPIPF_ENOMEM, "the accumulator needs %zu bytes (2 x %d chains x %d columns x %d int32): hipMalloc failed",
                        need, S, F, N);
        }
        c->inc_acc_bytes = need;
    }
    return 0;
}

// Negative-binomial reporting.  negbin_check: a chain's dispersion and probs.  The device's log is
// defined for normal doubles, so besides the model's own domain (dispersion in (0, 1e6], probs finite and >= 0) a
// subnormal dispersion, a subnormal probs and a probs beyond 2^990 (whose mean probs x flow could overflow) are refused.
// negbin_constants: the host's share of the factor, c(y, kappa) per (chain, row, column) and (kappa, log kappa) per
// chain (negbin_coefficients, logfact.cpp), copied to the device buffers the kNegBin kernels read.
constexpr double kNegBinMaxDispersion = 1e6;
static int negbin_check(int ch, double kappa, double pr) {
    if (!(kappa > 0.0 && kappa < INFINITY))
        return fail(EPIPF_EINVAL, "dispersion[%d]=%g: the dispersion must be finite and > 0", ch, kappa);
    if (kappa > kNegBinMaxDispersion)
        return fail(EPIPF_EINVAL, "dispersion[%d]=%g: above 1e6 the factor's rounding error grows with the dispersion; the Poisson limit beyond it is out of scope", ch, kappa);
    if (kappa < DBL_MIN) return fail(EPIPF_EINVAL, "dispersion[%d]=%g: a subnormal dispersion is out of scope", ch, kappa);
    if (!(pr >= 0.0 && pr < INFINITY))
        return fail(EPIPF_EINVAL, "probs[%d]=%g: the reporting ratio must be finite and >= 0", ch, pr);
    if ((pr > 0.0 && pr < DBL_MIN) || pr > 0x1.0p990)
        return fail(EPIPF_EINVAL, "probs[%d]=%g: a reporting ratio that is subnormal or above 2^990 is out of scope", ch, pr);
    return 0;
}

static int ensure_doubles(epipf_ctx* c, double*& buf, size_t& have, size_t n) {
    if (n > have) {
        if (buf) { (void)hipStreamSynchronize(c->stream); (void)hipFree(buf); }
        buf = nullptr;
        have = 0;
        if (dalloc(&buf, n)) return EPIPF_ENOMEM;
        have = n;
    }
    return 0;
}

// rows [T][F] (NaN: not reported), dispersion [S] (checked).  coeff and chain stay alive until the stream is synchronised.
static int negbin_constants(epipf_ctx* c, const std::vector<double>& rows, int S, int T, int F, const double* dispersion,
                            std::vector<double>& coeff, std::vector<double>& chain, NegBinArgs& nb) {
    coeff.resize((size_t)S * T * F);
    chain.resize((size_t)S * 2);
    for (int s = 0; s < S; ++s) {
        chain[2 * (size_t)s] = dispersion[s];
        chain[2 * (size_t)s + 1] = std::log(dispersion[s]);
    }
    negbin_coefficients(rows.data(), (size_t)T * F, dispersion, S, coeff.data());
    if (const int e = ensure_doubles(c, c->nb_coeff, c->nb_coeff_n, coeff.size())) return e;
    if (const int e = ensure_doubles(c, c->nb_chain, c->nb_chain_n, chain.size())) return e;
    HIP_TRY(hipMemcpyAsync(c->nb_coeff, coeff.data(), sizeof(double) * coeff.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->nb_chain, chain.data(), sizeof(double) * chain.size(), hipMemcpyHostToDevice, c->stream));
    nb.coeff = c->nb_coeff;
    nb.chain = c->nb_chain;
    return 0;
}

int epipf_negbin_coefficients(const double* y, int n, double dispersion, double* out) {
    if (n < 0 || (n > 0 && (!y || !out))) return fail(EPIPF_EINVAL, "NULL argument");
    if (!(dispersion > 0.0 && dispersion <= kNegBinMaxDispersion))
        return fail(EPIPF_EINVAL, "dispersion=%g outside (0, 1e6]", dispersion);
    for (int i = 0; i < n; ++i)
        if (!(y[i] >= 0.0 && y[i] < INFINITY && y[i] == std::floor(y[i])))
            return fail(EPIPF_EINVAL, "y[%d]=%g: a report must be an integer >= 0", i, y[i]);
    negbin_coefficients(y, (size_t)n, &dispersion, 1, out);
    return EPIPF_OK;
}

// The filter on reported transition counts: T = D + 2 rows (row 0 the initial draw, rows 1..D the days, row D + 1 one more
// resampling on day D's weights), weights from the particles' flows (epipf_incidence.hpp).  hidden, ancestry, status and
// log_zeta are the context's own and the run length becomes D + 2, so epipf_copy_history, epipf_path_sample, epipf_smooth
// and epipf_smooth_lag see the pass afterwards.
// dispersion: null, or [n_chains] with obs_model = EPIPF_OBS_NEGBIN (epipf_run_incidence_negbin).
static int run_incidence(epipf_ctx* c, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                         const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, const double* counts,
                         int D, int cumulate, double* log_zetas_out, int32_t* status_out, const double* dispersion) {
    if (!c || !theta || !probs || !keys || !filter_index || !counts || !log_zetas_out || !status_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (c->model != EPIPF_SIR && c->model != EPIPF_SEIR)
        return fail(EPIPF_EINVAL, "incidence observations cover the SIR and SEIR models; the subgroup models are out of their scope");
    if (!c->have_pop) return fail(EPIPF_ESTATE, "epipf_set_population was not called");
    const int S = n_chains, N = c->N, F = incidence_flows(c->model);
    if (S < 1 || S > c->max_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, max_chains=%d]", S, c->max_chains);
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta has %d entries per chain, model needs %d", d, theta_dim(c->model, c->G));
    if (obs_model != EPIPF_OBS_BINOMIAL && obs_model != EPIPF_OBS_NORMAL && !dispersion) return fail(EPIPF_EINVAL, "bad obs_model %d", obs_model);
    if (D < 1 || (long long)D + 2 > c->Tmax) return fail(EPIPF_EINVAL, "D=%d: D + 2 rows outside [3, t_max=%d]", D, c->Tmax);
    const int T = D + 2;
    std::vector<double> rows, nb_coeff, nb_chain;
    std::vector<uint8_t> rep;
    if (const int e = incidence_rows(counts, D, F, obs_model, rows, rep)) return e;
    for (int ch = 0; ch < S; ++ch) {
        const bool on = !active || active[ch];
        ChainParam& q = c->h_cp[ch];
        memset(&q, 0, sizeof q);
        for (int i = 0; i < d; ++i) {
            const double v = theta[(size_t)ch * d + i];
            if (on && !(v >= 0.0 && v < INFINITY))
                return fail(EPIPF_EINVAL, "theta[%d][%d]=%g: parameters must be finite and >= 0", ch, i, v);
            set_theta(q, nullptr, i, v);
        }
        const double pr = probs[ch];
        if (on)
            if (const int e = dispersion ? negbin_check(ch, dispersion[ch], pr) : incidence_probs(ch, pr, obs_model)) return e;
        set_chain_stream(c, q, pr, keys[ch], filter_index[ch]);
        q.skip = on ? 0 : 1;
        q.chosen = -1;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->walk_valid = false;                               // the history is this run's from here on
    c->inc_valid = false;
    if (const int e = ensure_incidence_counts(c, rows.size())) return e;
    const size_t acc_half = (size_t)S * F * N;
    if (cumulate)
        if (const int e = ensure_incidence_acc(c, S, F, N)) return e;
    // rows and rep stay alive past the stream synchronisation below
    HIP_TRY(hipMemcpyAsync(c->cp, c->h_cp, sizeof(ChainParam) * S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->inc_counts, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->log_zeta, 0xFF, sizeof(double) * (size_t)S * T, c->stream));   // rows never written read as NaN
    const size_t b_counters = sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride;
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));

    IncidenceArgs a{};
    StepArgs& s = a.s;
    one_lane_step_args(c, T, s);
    s.Y = nullptr;                                       // the reports are a.counts
    a.counts = c->inc_counts; a.acc = cumulate ? c->inc_acc : nullptr; a.acc_half = acc_half;

    NegBinArgs nb{};
    if (dispersion) {
        // a skipped chain's dispersion is not checked and not used: its constants are a valid chain's
        std::vector<double> kap(dispersion, dispersion + S);
        for (int ch = 0; ch < S; ++ch)
            if (active && !active[ch]) kap[ch] = 1.0;
        if (const int e = negbin_constants(c, rows, S, T, F, kap.data(), nb_coeff, nb_chain, nb)) return e;
    }
    FilterStreams fs{};
    if (const int e = fork_streams(c, std::min(c->n_streams, S), fs)) return e;
    const hipError_t le = launch_incidence(a, c->model, obs_model, cumulate != 0, rep.data(), S, fs, dispersion ? &nb : nullptr);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(log_zetas_out, c->log_zeta, sizeof(double) * (size_t)S * T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->status, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_counters, c->counters, b_counters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    harvest_counters(c, s.count_events != 0, false);
    // a chain that died at step p wrote -inf there and nothing after: its later rows are -inf as well; a skipped chain
    // ran nothing: NaN throughout (epipf_run)
    int n_active = 0;
    for (int q = 0; q < S; ++q) {
        n_active += status_out[q] != EPIPF_STATUS_SKIPPED;
        for (int p = 0; p < T; ++p) {
            double& v = log_zetas_out[(size_t)q * T + p];
            if (status_out[q] == EPIPF_STATUS_SKIPPED) v = NAN;
            else if (status_out[q] == EPIPF_STATUS_DEGENERATE && std::isnan(v)) v = -INFINITY;
        }
    }
    c->stats.particle_steps += (int64_t)n_active * N * T;
    c->stats.filters += n_active;
    c->stats.last_lanes = 1;
    c->stats.last_lane_events = 1;
    c->stats.last_fused = 0;
    c->last_chains = S;
    c->last_T = T;
    c->have_run = true;
    c->inc_valid = true;
    return EPIPF_OK;
}

int epipf_run_incidence(epipf_ctx* c, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                        const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, const double* counts,
                        int D, int cumulate, double* log_zetas_out, int32_t* status_out) {
    return run_incidence(c, n_chains, theta, d, obs_model, probs, keys, filter_index, active, counts, D, cumulate,
                         log_zetas_out, status_out, nullptr);
}

int epipf_run_incidence_negbin(epipf_ctx* c, int n_chains, const double* theta, int d, const double* probs,
                               const double* dispersion, const uint64_t* keys, const uint32_t* filter_index,
                               const int32_t* active, const double* counts, int D, int cumulate, double* log_zetas_out,
                               int32_t* status_out) {
    if (!dispersion) return fail(EPIPF_EINVAL, "NULL argument");
    return run_incidence(c, n_chains, theta, d, EPIPF_OBS_NEGBIN, probs, keys, filter_index, active, counts, D, cumulate,
                         log_zetas_out, status_out, dispersion);
}

// ------------------------------------------------------------------------ R_t from case counts
// The random-walk filter on reported transition counts: epipf_walk_filter's swarm, half-widths and theta_hist under
// epipf_run_incidence's rows, reports and accumulator (epipf_walk_incidence.hpp).  The run length becomes D + 2 and the
// parameter history is the context's, so the history calls of both parents see the pass afterwards.
// dispersion: null, or [n_chains] with obs_model = EPIPF_OBS_NEGBIN (epipf_incidence_walk_negbin).
static int incidence_walk(epipf_ctx* c, int n_chains, const double* swarm_in, int d, const double* half_widths, int obs_model,
                          const double* probs, const uint64_t* keys, const uint32_t* filter_index, const double* counts,
                          int D, int cumulate, double* log_zetas_out, int32_t* status_out, const double* dispersion) {
    if (!c || !swarm_in || !half_widths || !probs || !keys || !filter_index || !counts || !log_zetas_out || !status_out)
        return fail(EPIPF_EINVAL, "NULL argument");
    if (c->model != EPIPF_SIR && c->model != EPIPF_SEIR)
        return fail(EPIPF_EINVAL, "the random-walk filter on incidence covers the SIR and SEIR models; the subgroup models are out of its scope");
    if (!c->have_pop) return fail(EPIPF_ESTATE, "epipf_set_population was not called");
    const int S = n_chains, N = c->N, F = incidence_flows(c->model);
    if (d != theta_dim(c->model, c->G)) return fail(EPIPF_EINVAL, "theta has %d entries per particle, model needs %d", d, theta_dim(c->model, c->G));
    if (S < 1 || S > c->max_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, max_chains=%d]", S, c->max_chains);
    if (obs_model != EPIPF_OBS_BINOMIAL && obs_model != EPIPF_OBS_NORMAL && !dispersion) return fail(EPIPF_EINVAL, "bad obs_model %d", obs_model);
    if (D < 1 || (long long)D + 2 > c->Tmax) return fail(EPIPF_EINVAL, "D=%d: D + 2 rows outside [3, t_max=%d]", D, c->Tmax);
    const int T = D + 2;
    if (const int e = check_swarm(half_widths, (size_t)S, swarm_in, (size_t)S, N, d)) return e;
    std::vector<double> rows, nb_coeff, nb_chain;
    std::vector<uint8_t> rep;
    if (const int e = incidence_rows(counts, D, F, obs_model, rows, rep)) return e;
    for (int s = 0; s < S; ++s) {
        if (const int e = dispersion ? negbin_check(s, dispersion[s], probs[s]) : incidence_probs(s, probs[s], obs_model)) return e;
        ChainParam& q = c->h_cp[s];
        memset(&q, 0, sizeof q);                         // theta is the particles' own
        set_chain_stream(c, q, probs[s], keys[s], filter_index[s]);
        q.chosen = -1;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->walk_valid = false;                               // the history is this call's from here on
    c->inc_valid = false;
    const size_t comp = (size_t)d * N, stride = (size_t)T * comp;
    if (const int e = ensure_walk_theta(c, S, T, d, N)) return e;
    if (const int e = ensure_incidence_counts(c, rows.size())) return e;
    const size_t acc_half = (size_t)S * F * N;
    if (cumulate)
        if (const int e = ensure_incidence_acc(c, S, F, N)) return e;
    // scratch: start [S][d][N] | hw [S][d]
    const size_t b_start = align256(sizeof(double) * (size_t)S * comp), b_hw = align256(sizeof(double) * (size_t)S * d);
    if (ensure_scratch(c, b_start + b_hw)) return EPIPF_ENOMEM;
    double* d_start = (double*)c->scratch;
    double* d_hw = (double*)((char*)c->scratch + b_start);
    std::vector<double> soa((size_t)S * comp);            // [S][N][d] -> [S][d][N]
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < d; ++k) soa[((size_t)s * d + k) * N + j] = swarm_in[((size_t)s * N + j) * d + k];
    // rows, rep and soa stay alive past the stream synchronisation below
    HIP_TRY(hipMemcpyAsync(c->cp, c->h_cp, sizeof(ChainParam) * S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_start, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_hw, half_widths, sizeof(double) * (size_t)S * d, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->inc_counts, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->log_zeta, 0xFF, sizeof(double) * (size_t)S * T, c->stream));   // rows never written read as NaN
    const size_t b_counters = sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride;
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));

    WalkIncidenceArgs a{};
    StepArgs& s = a.s;
    one_lane_step_args(c, T, s);
    s.Y = nullptr;                                       // the reports are a.counts
    a.d = d; a.hw = d_hw; a.start = d_start; a.hist = c->walk_theta; a.chain_stride = stride;
    a.counts = c->inc_counts; a.acc = cumulate ? c->inc_acc : nullptr; a.acc_half = acc_half;

    NegBinArgs nb{};
    if (dispersion)
        if (const int e = negbin_constants(c, rows, S, T, F, dispersion, nb_coeff, nb_chain, nb)) return e;
    FilterStreams fs{};
    if (const int e = fork_streams(c, std::min(c->n_streams, S), fs)) return e;
    const hipError_t le = launch_walk_incidence(a, c->model, obs_model, cumulate != 0, rep.data(), S, fs, dispersion ? &nb : nullptr);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(log_zetas_out, c->log_zeta, sizeof(double) * (size_t)S * T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->status, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_counters, c->counters, b_counters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, b_counters, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    harvest_counters(c, s.count_events != 0, false);
    // a chain that died at step p wrote -inf there and nothing after: its later rows are -inf as well
    for (int q = 0; q < S; ++q)
        if (status_out[q] == EPIPF_STATUS_DEGENERATE)
            for (int p = 0; p < T; ++p)
                if (std::isnan(log_zetas_out[(size_t)q * T + p])) log_zetas_out[(size_t)q * T + p] = -INFINITY;
    c->stats.particle_steps += (int64_t)S * N * T;
    c->stats.filters += S;
    c->stats.last_lanes = 1;
    c->stats.last_lane_events = 1;
    c->stats.last_fused = 0;
    c->last_chains = S;
    c->last_T = T;
    c->have_run = true;
    c->walk_valid = true;
    c->inc_valid = true;
    trim_scratch(c);
    return EPIPF_OK;
}

int epipf_incidence_walk(epipf_ctx* c, int n_chains, const double* swarm_in, int d, const double* half_widths, int obs_model,
                         const double* probs, const uint64_t* keys, const uint32_t* filter_index, const double* counts,
                         int D, int cumulate, double* log_zetas_out, int32_t* status_out) {
    return incidence_walk(c, n_chains, swarm_in, d, half_widths, obs_model, probs, keys, filter_index, counts, D, cumulate,
                          log_zetas_out, status_out, nullptr);
}

int epipf_incidence_walk_negbin(epipf_ctx* c, int n_chains, const double* swarm_in, int d, const double* half_widths,
                                const double* probs, const double* dispersion, const uint64_t* keys,
                                const uint32_t* filter_index, const double* counts, int D, int cumulate,
                                double* log_zetas_out, int32_t* status_out) {
    if (!dispersion) return fail(EPIPF_EINVAL, "NULL argument");
    return incidence_walk(c, n_chains, swarm_in, d, half_widths, EPIPF_OBS_NEGBIN, probs, keys, filter_index, counts, D,
                          cumulate, log_zetas_out, status_out, dispersion);
}

// The smoothed true flows of the last incidence pass: the flows of every particle formed on the device from the
// resident history (launch_incidence_flows, into smooth_run's scratch) and reduced by the smoother's kernels as a
// history of F compartments under the genealogy's multiplicities.
int epipf_incidence_smooth(epipf_ctx* c, int n_chains, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                           int32_t* quant_out, int32_t* lineages_out) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (!c->inc_valid)
        return fail(EPIPF_ESTATE, c->have_run ? "the context's history is no longer an incidence pass's: another run overwrote it"
                                              : "no incidence pass has run on this context");
    if (n_chains < 1 || n_chains > c->last_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->last_chains);
    return smooth_run(c, n_chains, c->last_T, c->N, incidence_flows(c->model), nullptr, nullptr, EPIPF_LINEAGE_GENEALOGY,
                      EPIPF_SMOOTH_SMOOTHING, lag < 0 ? kSmoothNoLag : lag, q, n_q, bins, sums_out, quant_out, lineages_out,
                      true);
}

static int walk_state(const epipf_ctx* c, int n_chains) {
    if (!c->walk_valid)
        return fail(EPIPF_ESTATE, c->have_run ? "the context's history is no longer a random-walk filter's: another run overwrote it"
                                              : "no random-walk filter has run on this context");
    if (n_chains < 1 || n_chains > c->last_chains) return fail(EPIPF_EINVAL, "n_chains=%d outside [1, %d]", n_chains, c->last_chains);
    return 0;
}

// theta_out [n][T][N][d]; the rows of a degenerate chain from its dying step on are NaN (the device never wrote them).
int epipf_walk_history(epipf_ctx* c, int n_chains, double* theta_out) {
    if (!c || !theta_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (int rc = walk_state(c, n_chains)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int T = c->last_T, N = c->N, d = theta_dim(c->model, c->G);
    const size_t stride = (size_t)T * d * N;
    std::vector<double> soa((size_t)n_chains * stride), lz((size_t)n_chains * T);
    std::vector<int32_t> st((size_t)n_chains);
    HIP_TRY(hipMemcpyAsync(soa.data(), c->walk_theta, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(lz.data(), c->log_zeta, sizeof(double) * lz.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(st.data(), c->status, sizeof(int32_t) * st.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int s = 0; s < n_chains; ++s) {
        int alive = T;                                   // days whose rows were written
        if (st[s] != EPIPF_STATUS_OK)
            for (alive = 0; alive < T && lz[(size_t)s * T + alive] > -INFINITY; ++alive) {}
        for (int p = 0; p < T; ++p)
            for (int j = 0; j < N; ++j)
                for (int k = 0; k < d; ++k)
                    theta_out[(((size_t)s * T + p) * N + j) * d + k] =
                        p < alive ? soa[(size_t)s * stride + ((size_t)p * d + k) * N + j] : NAN;
    }
    return EPIPF_OK;
}

// The reduction over n chains: the context's own history and theta_hist (up_hidden == NULL) or the caller's arrays,
// uploaded to scratch with theta already [n][T][d][N].  One workgroup per (chain, day); chains and days are sliced so
// that the global multiplicity rows of a launch (N > kSmoothLdsMaxN) stay within the smoother's scratch budget.
static int walk_smooth_run(epipf_ctx* c, int n, int T, int N, int C, int d, double pop, const int32_t* up_hidden,
                           const int32_t* up_ancestry, const double* up_theta, int lineage, int lag, const double* q, int n_q,
                           double* mean_out, double* quant_out, int32_t* lineages_out) {
    if (!mean_out || !lineages_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (lineage != EPIPF_LINEAGE_REFERENCE && lineage != EPIPF_LINEAGE_GENEALOGY)
        return fail(EPIPF_EINVAL, "unknown lineage %d", lineage);
    if (n_q < 0 || (n_q > 0 && !q)) return fail(EPIPF_EINVAL, "n_q=%d needs q", n_q);
    if (n_q > 0 && !quant_out) return fail(EPIPF_EINVAL, "quantiles need quant_out");
    for (int i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(EPIPF_EINVAL, "q[%d] must lie in [0, 1]", i);
    if (N > kSmoothMaxN) return fail(EPIPF_EINVAL, "at most %d particles, got %d", kSmoothMaxN, N);
    if (lag < 0 || lag > T - 1) lag = T - 1;              // "full"
    const int V = d + 1;
    bool lds_rows = N <= kSmoothLdsMaxN;
    if (const char* e = getenv("EPIPF_SMOOTH_LDS")) lds_rows = lds_rows && atoi(e) != 0;
    const size_t rb1 = lds_rows ? 0 : 2 * sizeof(uint32_t) * (size_t)N;   // one workgroup's global rows
    size_t budget = kSmoothScratch;
    if (const char* e = getenv("EPIPF_SMOOTH_SCRATCH_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    int days = T;
    if (rb1 > 0 && (size_t)T * rb1 > budget) days = (int)std::max<size_t>(1, std::min<size_t>((size_t)T, budget / rb1));
    days = std::min(days, kSmoothLagMaxBlocks);
    int slice = n;
    if (rb1 > 0) slice = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, budget / ((size_t)days * rb1)));
    slice = std::min(slice, std::max(1, kSmoothLagMaxBlocks / days));
    HIP_TRY(hipSetDevice(c->device));
    const size_t ob_m = align256(sizeof(double) * (size_t)n * T * V);
    const size_t ob_q = n_q > 0 ? align256(sizeof(double) * (size_t)n * n_q * T * V) : 0;
    const size_t ob_l = align256(sizeof(int32_t) * (size_t)n * T);
    const size_t ob_r = n_q > 0 ? align256(sizeof(uint32_t) * (size_t)n_q) : 0;
    const size_t sb_m = align256((size_t)slice * days * rb1);
    const size_t ub_h = up_hidden ? align256(sizeof(int32_t) * (size_t)n * T * N * C) : 0;
    const size_t ub_a = up_hidden ? align256(sizeof(int32_t) * (size_t)n * T * N) : 0;
    const size_t ub_t = up_hidden ? align256(sizeof(double) * (size_t)n * T * N * d) : 0;
    if (ensure_scratch(c, ob_m + ob_q + ob_l + ob_r + sb_m + ub_h + ub_a + ub_t)) return EPIPF_ENOMEM;
    char* p = (char*)c->scratch;
    double* dmean = (double*)p; p += ob_m;
    double* dquant = (double*)p; p += ob_q;
    int32_t* dlin = (int32_t*)p; p += ob_l;
    uint32_t* dranks = (uint32_t*)p; p += ob_r;
    uint32_t* drows = (uint32_t*)p; p += sb_m;
    int32_t* dhid = (int32_t*)p; p += ub_h;
    int32_t* danc = (int32_t*)p; p += ub_a;
    double* dth = (double*)p;
    HIP_TRY(hipMemsetAsync(dmean, 0, ob_m + ob_q + ob_l, c->stream));
    std::vector<uint32_t> ranks((size_t)n_q);
    for (int i = 0; i < n_q; ++i) ranks[i] = (uint32_t)std::max(std::ceil(q[i] * (double)N), 1.0);   // inverted_cdf, q N in float64
    if (n_q > 0) HIP_TRY(hipMemcpyAsync(dranks, ranks.data(), sizeof(uint32_t) * n_q, hipMemcpyHostToDevice, c->stream));
    WalkSmoothArgs a{};
    a.T = T; a.N = N; a.C = C; a.d = d; a.shift = lineage == EPIPF_LINEAGE_GENEALOGY ? 1 : 0; a.lag = lag; a.n_q = n_q;
    a.pop = pop; a.ranks = n_q > 0 ? dranks : nullptr; a.mean = dmean; a.quant = dquant; a.lineages = dlin;
    if (up_hidden) {
        HIP_TRY(hipMemcpyAsync(dhid, up_hidden, sizeof(int32_t) * (size_t)n * T * N * C, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(danc, up_ancestry, sizeof(int32_t) * (size_t)n * T * N, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dth, up_theta, sizeof(double) * (size_t)n * T * N * d, hipMemcpyHostToDevice, c->stream));
        a.hidden = dhid; a.ancestry = danc; a.theta = dth; a.status = nullptr;
        a.hist_stride = (size_t)T * N * C; a.anc_stride = (size_t)T * N; a.theta_stride = (size_t)T * N * d;
    } else {
        a.hidden = c->hidden; a.ancestry = c->ancestry; a.theta = c->walk_theta; a.status = c->status;
        a.hist_stride = c->hist_stride; a.anc_stride = c->anc_stride; a.theta_stride = (size_t)T * N * d;
    }
    for (int c0 = 0; c0 < n; c0 += slice) {
        a.n = std::min(slice, n - c0);
        a.chain0 = c0;
        a.mrows = rb1 ? drows : nullptr;
        for (int d0 = 0; d0 < T; d0 += days) {
            a.day0 = d0;
            a.days = std::min(days, T - d0);
            const hipError_t le = launch_walk_smooth(a, c->stream);
            if (le != hipSuccess) return fail(EPIPF_EHIP, "walk smooth launch failed: %s", hipGetErrorString(le));
        }
    }
    HIP_TRY(hipMemcpyAsync(mean_out, dmean, sizeof(double) * (size_t)n * T * V, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(lineages_out, dlin, sizeof(int32_t) * (size_t)n * T, hipMemcpyDeviceToHost, c->stream));
    if (n_q > 0)
        HIP_TRY(hipMemcpyAsync(quant_out, dquant, sizeof(double) * (size_t)n * n_q * T * V, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    trim_scratch(c);
    return EPIPF_OK;
}

int epipf_walk_smooth(epipf_ctx* c, int n_chains, int lineage, int lag, const double* q, int n_q, double* mean_out,
                      double* quant_out, int32_t* lineages_out) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (int rc = walk_state(c, n_chains)) return rc;
    return walk_smooth_run(c, n_chains, c->last_T, c->N, c->C, theta_dim(c->model, c->G), c->npop[0], nullptr, nullptr,
                           nullptr, lineage, lag, q, n_q, mean_out, quant_out, lineages_out);
}

int epipf_walk_smooth_history(epipf_ctx* c, int n, int T, int N, int C, int d, const int32_t* hidden,
                              const int32_t* ancestry, const double* theta, double population_total, int lineage, int lag,
                              const double* q, int n_q, double* mean_out, double* quant_out, int32_t* lineages_out) {
    if (!c || !hidden || !ancestry || !theta) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 1 || T < 1 || N < 1 || C < 1) return fail(EPIPF_EINVAL, "n, T, N, C must be >= 1");
    if (d < 1 || d > kIf2MaxD) return fail(EPIPF_EINVAL, "d=%d outside [1, %d]", d, kIf2MaxD);
    if (!(population_total > 0.0 && population_total < INFINITY))
        return fail(EPIPF_EINVAL, "population_total=%g must be finite and > 0", population_total);
    if ((double)n * T * N * std::max(C, 2 * d) > (double)((size_t)1 << 40)) return fail(EPIPF_EINVAL, "history too large");
    const size_t TN = (size_t)T * N;
    for (size_t i = 0; i < (size_t)n * TN * d; ++i)
        if (!(theta[i] >= 0.0 && theta[i] < INFINITY))
            return fail(EPIPF_EINVAL, "theta[%zu][%zu][%zu][%zu]=%g: parameters must be finite and >= 0", i / (TN * d),
                        i / ((size_t)N * d) % T, i / d % N, i % d, theta[i]);
    for (size_t i = 0; i < (size_t)n * TN * C; ++i)
        if (hidden[i] < 0)
            return fail(EPIPF_EINVAL, "hidden[%zu][%zu][%zu][%zu]=%d: counts must be non-negative", i / (TN * C),
                        i / ((size_t)N * C) % T, i / C % N, i % C, hidden[i]);
    for (size_t i = 0; i < (size_t)n * TN; ++i)
        if (ancestry[i] < 0 || ancestry[i] >= N)
            return fail(EPIPF_EINVAL, "ancestry[%zu][%zu][%zu]=%d: ancestors must lie in [0, N)", i / TN, i / N % T, i % N,
                        ancestry[i]);
    std::vector<double> soa((size_t)n * TN * d);          // [n][T][N][d] -> [n][T][d][N]
    for (size_t r = 0; r < (size_t)n * T; ++r)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < d; ++k) soa[(r * d + k) * N + j] = theta[(r * N + j) * d + k];
    return walk_smooth_run(c, n, T, N, C, d, population_total, hidden, ancestry, soa.data(), lineage, lag, q, n_q, mean_out,
                           quant_out, lineages_out);
}

int epipf_glibc_log(int64_t n, const double* x, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(EPIPF_EINVAL, "NULL argument");
    LogTab lt[kLogTabEntries];
    glibc_log_table(lt);
    for (int64_t i = 0; i < n; ++i) out[i] = glibc_log_impl(x[i], lt);
    return EPIPF_OK;
}

int epipf_clock_log(int64_t n, const double* x, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(EPIPF_EINVAL, "NULL argument");
    LogTab lt[kLogTabEntries];
    glibc_log_table(lt);
    for (int64_t i = 0; i < n; ++i) out[i] = clock_log_impl(x[i], lt);
    return EPIPF_OK;
}

int epipf_resample(epipf_ctx* c, int n, const double* w, const double* u, int32_t* out, int64_t* fallbacks_out) {
    if (!c || !w || !u || !out) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 1) return fail(EPIPF_EINVAL, "n must be >= 1");
    const int B = (n + 255) / 256;
    if (step_lds_bytes(B, 256) > 160 * 1024) return fail(EPIPF_EINVAL, "n too large");
    for (int i = 0; i < n; ++i)
        if (!(u[i] >= 0.0 && u[i] < 1.0)) return fail(EPIPF_EINVAL, "uniforms must lie in [0, 1)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nw = align256(sizeof(double) * (size_t)B * 256);
    const size_t need = 4 * nw + align256(sizeof(double) * B) + align256(sizeof(int32_t) * (size_t)n) + 512;
    if (ensure_scratch(c, need)) return EPIPF_ENOMEM;
    char* p = (char*)c->scratch;
    ResampleArgs a{};
    a.N = n; a.B = B; a.cert_k = cert_k(n, B, prefix_segment(B), 256);
    double* dw = (double*)p; p += nw;
    double* du = (double*)p; p += nw;
    a.wraw = (double*)p; p += nw;
    a.wloc = (double*)p; p += nw;
    a.bsum = (double*)p; p += align256(sizeof(double) * B);
    a.out = (int32_t*)p; p += align256(sizeof(int32_t) * (size_t)n);
    a.status = (int32_t*)p; p += 256;
    a.fallbacks = (unsigned long long*)p;
    a.w = dw; a.u = du;
    HIP_TRY(hipMemcpyAsync(dw, w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(du, u, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(a.status, 0, 256 + sizeof(unsigned long long), c->stream));
    hipError_t le = launch_resample(a, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "resample launch failed: %s", hipGetErrorString(le));
    int32_t st = 0;
    unsigned long long fb = 0;
    HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&st, a.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&fb, a.fallbacks, sizeof fb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fallbacks_out) *fallbacks_out = (int64_t)fb;
    return st ? EPIPF_STATUS_DEGENERATE : EPIPF_OK;
}

// ------------------------------------------------------------------------------- ABC rejection
namespace {
struct AbcPlan {
    AbcArgs args{};
    double* Ydev = nullptr;
    int32_t* idx = nullptr;
    int32_t* count = nullptr;
    double* traj = nullptr;
    double* theta_out = nullptr;
    double* dist_out = nullptr;       // [samples] accepted distances
    int32_t* anc_out = nullptr;       // [samples] accepted ancestors
    int32_t* anc = nullptr;           // [batch] ABC-SMC ancestors of the batch
    double* prev_theta = nullptr;     // [n_prev][2] ABC-SMC previous population
    double* prev_cdf = nullptr;       // [n_prev]
};

// Validates the reference-level arguments and fills the launch constants (abc_algo.py:35-39).
int abc_prepare(epipf_ctx* c, const double* Y, int T, const double* priors, uint64_t key, uint32_t run_index,
                AbcArgs& a) {
    if (!c || !Y || !priors) return fail(EPIPF_EINVAL, "NULL argument");
    if (T < 1 || T > kAbcMaxDays) return fail(EPIPF_EINVAL, "T=%d outside [1, %d]", T, kAbcMaxDays);
    for (int q = 0; q < 4; ++q)
        if (!(priors[q] >= 0.0 && priors[q] < INFINITY))
            return fail(EPIPF_EINVAL, "priors[%d]=%g: prior bounds must be finite and >= 0", q, priors[q]);
    for (int q = 0; q < 3 * T; ++q)
        if (!std::isfinite(Y[q])) return fail(EPIPF_EINVAL, "observed_data[%d][%d] is not finite", q / 3, q % 3);
    memset(&a, 0, sizeof a);
    for (int j = 0; j < 2; ++j) {
        a.prior_lo[j] = priors[2 * j];
        a.prior_rng[j] = priors[2 * j + 1] - priors[2 * j];           // numpy uniform: low + (high - low) * U
    }
    for (int q = 0; q < 3; ++q) {
        const double lam = std::trunc(Y[q]);                           // Y[0].astype(int), :38
        if (lam < 0.0) return fail(EPIPF_EINVAL, "observed_data[0][%d]=%g: Poisson lam < 0 (numpy raises)", q, Y[q]);
        if (lam > 1e9) return fail(EPIPF_EINVAL, "observed_data[0][%d]=%g: initial count above 1e9", q, Y[q]);
        a.lam[q] = lam;
        a.pm[q] = lam > 0.0 ? std::exp(-lam + lam * std::log(lam) - std::lgamma(lam + 1.0)) : 0.0;   // host glibc
    }
    a.T = T;
    a.reject_sum = INFINITY;                                           // early rejection: epipf_abc turns it on
    a.last_day = (double)(T - 1);
    a.f = run_index;
    a.k0 = (uint32_t)key;
    a.k1 = (uint32_t)(key >> 32);
    a.logtab = c->logtab;
    a.counters = c->counters;
    a.count = c->profiling >= EPIPF_PROFILE_COUNTERS ? 1 : 0;
    c->abc_order = true;
    if (const char* e = getenv("EPIPF_ABC_ORDER")) c->abc_order = atoi(e) != 0;
    // lane groups for the longest trials (abc_trials_group_kernel): W lanes each for the first `abc_frac` of
    // the sorted trials; EPIPF_ABC_LANES = 1 turns them off (results are identical either way)
    a.group_lanes = c->abc_lanes;                                      // 0: chosen per launch (abc_launch_trials)
    if (const char* e = getenv("EPIPF_ABC_LANES")) {
        const int w = atoi(e);
        if (w == 1 || w == 2 || w == 4 || w == 8 || w == 16) a.group_lanes = w;
    }
    c->abc_frac = -1.0;
    if (const char* e = getenv("EPIPF_ABC_GROUP_FRAC")) c->abc_frac = atof(e) < 0.0 ? -1.0 : std::min(1.0, atof(e));
    return 0;
}

// Carves the ABC buffers for batches of up to `batch` trials and `samples` output slots (n_prev: the previous
// population of an ABC-SMC generation, else 0).
int abc_buffers(epipf_ctx* c, int T, int batch, int samples, AbcPlan& p, int n_prev = 0) {
    const size_t b = (size_t)batch;
    const size_t sz_do = align256(sizeof(double) * (size_t)samples), sz_ao = align256(sizeof(int32_t) * (size_t)samples),
                 sz_anc = align256(sizeof(int32_t) * b), sz_pt = align256(sizeof(double) * 2 * (size_t)n_prev),
                 sz_pc = align256(sizeof(double) * (size_t)n_prev);
    const size_t sz_days = align256(sizeof(int32_t) * 3 * (size_t)T * b), sz_theta = align256(sizeof(double) * 2 * b),
                 sz_dist = align256(sizeof(double) * b), sz_Y = align256(sizeof(double) * 3 * (size_t)T),
                 sz_idx = align256(sizeof(int32_t) * (size_t)(samples + 1)), sz_cnt = 256,
                 sz_traj = align256(sizeof(double) * 4 * (size_t)T * samples), sz_to = align256(sizeof(double) * 2 * (size_t)samples);
    const size_t sz_key = align256(sizeof(uint32_t) * b), sz_tmp = align256(abc_sort_temp_bytes(batch));
    const size_t need = sz_days + sz_theta + sz_dist + sz_Y + sz_idx + sz_cnt + sz_traj + sz_to + 4 * sz_key + sz_tmp +
                        sz_do + sz_ao + sz_anc + sz_pt + sz_pc;
    if (need > c->abc_bytes) {
        if (c->abc) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->abc); c->abc = nullptr; c->abc_bytes = 0; }
        if (hipMalloc(&c->abc, need) != hipSuccess) return fail(EPIPF_ENOMEM, "ABC buffers hipMalloc(%zu) failed", need);
        c->abc_bytes = need;
    }
    char* q = (char*)c->abc;
    p.args.days = (int32_t*)q; q += sz_days;
    p.args.theta = (double*)q; q += sz_theta;
    p.args.dist = (double*)q; q += sz_dist;
    p.Ydev = (double*)q; q += sz_Y;
    p.idx = (int32_t*)q; q += sz_idx;
    p.count = (int32_t*)q; q += sz_cnt;
    p.traj = (double*)q; q += sz_traj;
    p.theta_out = (double*)q; q += sz_to;
    for (int k = 0; k < 2; ++k) {
        p.args.sort_keys[k] = (uint32_t*)q; q += sz_key;
        p.args.sort_vals[k] = (int32_t*)q; q += sz_key;
    }
    p.args.sort_temp = q; q += sz_tmp;
    p.args.sort_temp_bytes = sz_tmp;
    p.dist_out = (double*)q; q += sz_do;
    p.anc_out = (int32_t*)q; q += sz_ao;
    p.anc = (int32_t*)q; q += sz_anc;
    p.prev_theta = (double*)q; q += sz_pt;
    p.prev_cdf = (double*)q; q += sz_pc;
    p.args.perm = c->abc_order ? p.args.sort_vals[1] : nullptr;
    p.args.Y = p.Ydev;
    return 0;
}

// Launches of up to this many trials put the longest half on lane groups of 4 (automatic mode).  Measured at the
// reference's setting (profiles/r3_abc_lane_groups.jsonl): 64k-trial launches 5.0 -> 3.1 ms (+61% end to end), 128k
// +14%, 192k +3.5%.  Larger launches are throughput-bound and take lane groups only for the longest few percent: with
// round 4's lane-group kernel (fixed-point decisions, early rejection on groups) W = 16 on the longest 4% of a 256k
// launch runs the reference's setting at 3.06-3.08e7 trials/s against 2.90-2.93e7 one lane (3-8%: 3.0-3.07e7; W = 4
// or 8, 10% and more lose; profiles/r4q_abc_groups.txt).
constexpr int kAbcGroupMaxTrials = 196608;
constexpr int kAbcLongLanes = 16;
constexpr double kAbcLongFrac = 0.04;

int abc_launch_trials(epipf_ctx* c, AbcArgs& a0, uint32_t t0, int n) {
    AbcArgs& a = a0;
    a.t0 = t0;
    a.n = n;
    const int lanes = a.group_lanes;
    if (lanes == 0) a.group_lanes = n <= kAbcGroupMaxTrials ? 4 : kAbcLongLanes;
    const double frac = c->abc_frac >= 0.0 ? c->abc_frac : n <= kAbcGroupMaxTrials ? 0.5 : kAbcLongFrac;
    a.group_end = (a.group_lanes > 1 && a.perm) ? (int)std::llround(frac * n) : 0;
    if (a.group_end > 0 && !ensure_streams(c, 2)) return fail(EPIPF_EHIP, "auxiliary stream creation failed");
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipError_t le = launch_abc_trials(a, c->stream, a.group_end > 0 ? c->aux[1] : nullptr, c->fork, c->join[1]);
    a.group_lanes = lanes;                                             // automatic again for the next launch
    if (le != hipSuccess) return fail(EPIPF_EHIP, "ABC trial kernel launch failed: %s", hipGetErrorString(le));
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    return 0;
}

// An ABC-SMC batch: every trial on one lane after the sort
int abc_launch_smc_trials(epipf_ctx* c, AbcArgs& a, const AbcSmcArgs& m, uint32_t t0, int n) {
    a.t0 = t0;
    a.n = n;
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipError_t le = launch_abc_smc_trials(a, m, c->stream);
    if (le != hipSuccess) return fail(EPIPF_EHIP, "ABC-SMC trial kernel launch failed: %s", hipGetErrorString(le));
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    return 0;
}

int abc_account(epipf_ctx* c, int n) {
    if (c->profiling) {
        HIP_TRY(hipEventSynchronize(c->ev[1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        c->stats.abc_ms += ms;
    }
    c->stats.abc_launches += 1;
    c->stats.abc_trials += n;
    return 0;
}

int abc_read_counters(epipf_ctx* c) {
    if (c->profiling < EPIPF_PROFILE_COUNTERS) return 0;
    HIP_TRY(hipMemcpyAsync(c->h_counters, c->counters, sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride,
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long tot[kNumCounters] = {};
    for (int sl = 0; sl < kCounterSlots; ++sl)
        for (int k = 0; k < kNumCounters; ++k) tot[k] += c->h_counters[(size_t)sl * kCounterStride + k];
    c->stats.events = (int64_t)tot[0];
    c->stats.lane_iterations = (int64_t)tot[2];
    c->stats.wave_lane_slots = (int64_t)tot[3];
    return 0;
}
}  // namespace

int epipf_abc_trials(epipf_ctx* c, const double* Y, int T, const double* priors, uint64_t key, uint32_t run_index,
                     uint32_t t0, int n, double* theta_out, int32_t* rows_out, double* dist_out, int64_t* events_out) {
    AbcPlan p;
    if (int rc = abc_prepare(c, Y, T, priors, key, run_index, p.args)) return rc;
    if (!theta_out) return fail(EPIPF_EINVAL, "theta_out is NULL");
    if (n < 0 || (uint64_t)t0 + (uint64_t)n > (1ull << 32)) return fail(EPIPF_EINVAL, "trials [t0, t0+n) must lie in [0, 2^32)");
    if (n == 0) { if (events_out) *events_out = 0; return EPIPF_OK; }
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = abc_buffers(c, T, n, 1, p)) return rc;
    AbcArgs a = p.args;
    HIP_TRY(hipMemcpyAsync(p.Ydev, Y, sizeof(double) * 3 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    unsigned long long ev_before = 0;
    const bool counting = a.count != 0;
    if (counting) {
        if (int rc = abc_read_counters(c)) return rc;
        ev_before = (unsigned long long)c->stats.events;
    }
    if (int rc = abc_launch_trials(c, a, t0, n)) return rc;
    std::vector<double> th((size_t)2 * n);
    HIP_TRY(hipMemcpyAsync(th.data(), a.theta, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out, a.dist, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    std::vector<int32_t> days;
    if (rows_out) {
        days.resize((size_t)3 * T * n);
        HIP_TRY(hipMemcpyAsync(days.data(), a.days, sizeof(int32_t) * days.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = abc_account(c, n)) return rc;
    for (int i = 0; i < n; ++i) {
        theta_out[2 * (size_t)i] = th[i];
        theta_out[2 * (size_t)i + 1] = th[(size_t)n + i];
    }
    if (rows_out)   // device [T][3][n] -> caller [n][T][3]
        for (int d = 0; d < T; ++d)
            for (int q = 0; q < 3; ++q)
                for (int i = 0; i < n; ++i)
                    rows_out[((size_t)i * T + d) * 3 + q] = days[((size_t)d * 3 + q) * n + i];
    if (events_out) {
        *events_out = -1;
        if (counting) {
            if (int rc = abc_read_counters(c)) return rc;
            *events_out = (int64_t)((unsigned long long)c->stats.events - ev_before);
        }
    }
    return EPIPF_OK;
}

namespace {
// The previous population of an ABC-SMC generation (host pointers; n_prev = 0: the prior stage, none)
struct AbcSmcPrev {
    const double* theta;
    const double* cdf;
    int n_prev;
    const double* half_width;
};

// The accept loop of epipf_abc and of one ABC-SMC generation: trials t0, t0 + 1, ... in batches until no_of_samples
// are accepted or max_trials have run.  prev.n_prev = 0 draws theta from the prior (the rejection sampler, lane
// groups and all); otherwise from the previous population (launch_abc_smc_trials).  dist_out / ancestor_out may be
// NULL.  *trials_out counts from t0.
int abc_sample(epipf_ctx* c, const double* Y, int T, int no_of_samples, double threshold, const double* priors,
               const AbcSmcPrev& prev, uint64_t key, uint32_t run_index, uint32_t t0, int64_t max_trials, int batch,
               double* theta_out, double* traj_out, double* dist_out, int32_t* ancestor_out, int64_t* trials_out,
               int32_t* accepted_out) {
    AbcPlan p;
    if (int rc = abc_prepare(c, Y, T, priors, key, run_index, p.args)) return rc;
    if (!theta_out || !traj_out || !trials_out || !accepted_out) return fail(EPIPF_EINVAL, "NULL output pointer");
    if (no_of_samples < 0) return fail(EPIPF_EINVAL, "no_of_samples < 0");
    if (std::isnan(threshold)) return fail(EPIPF_EINVAL, "threshold is NaN");
    if (max_trials < 0 || max_trials > (int64_t)(1ull << 32)) return fail(EPIPF_EINVAL, "max_trials must lie in [0, 2^32]");
    if ((uint64_t)t0 + (uint64_t)max_trials > (1ull << 32))
        return fail(EPIPF_EINVAL, "t0 + max_trials = %llu exceeds 2^32", (unsigned long long)t0 + (unsigned long long)max_trials);
    if (batch < 0) return fail(EPIPF_EINVAL, "batch < 0");
    const int n_prev = prev.n_prev;
    if (n_prev > 0) {
        if (!prev.theta || !prev.cdf || !prev.half_width) return fail(EPIPF_EINVAL, "NULL previous population");
        // a proposal outside the prior box has distance +inf, which only a finite threshold rejects
        if (threshold == INFINITY) return fail(EPIPF_EINVAL, "threshold must be below +inf in an ABC-SMC generation");
        for (int q = 0; q < 2; ++q)
            if (!(prev.half_width[q] >= 0.0 && prev.half_width[q] < INFINITY))
                return fail(EPIPF_EINVAL, "half_width[%d]=%g: kernel half-widths must be finite and >= 0", q, prev.half_width[q]);
        for (int q = 0; q < 2 * n_prev; ++q)
            if (!std::isfinite(prev.theta[q])) return fail(EPIPF_EINVAL, "prev_theta[%d][%d] is not finite", q / 2, q % 2);
        if (!(prev.cdf[0] >= 0.0)) return fail(EPIPF_EINVAL, "prev_cdf[0]=%g: must be >= 0", prev.cdf[0]);
        for (int q = 1; q < n_prev; ++q)
            if (!(prev.cdf[q] >= prev.cdf[q - 1])) return fail(EPIPF_EINVAL, "prev_cdf is not non-decreasing at %d", q);
        if (prev.cdf[n_prev - 1] != 1.0) return fail(EPIPF_EINVAL, "prev_cdf ends at %.17g, not 1", prev.cdf[n_prev - 1]);
    }
    *trials_out = 0;
    *accepted_out = 0;
    if (no_of_samples == 0) return EPIPF_OK;
    // batch sizes: fixed, or 256k trials first, then 1.25x the trials the observed acceptance rate predicts for
    // the samples still missing (x4 while nothing is accepted), within [256k, 1M] and a day table < 4 GiB.  A launch
    // lasts at least as long as its longest trials (~5 ms at the reference's setting), and below ~4 waves per SIMD
    // the exact f64 trial loop is latency-bound: 64k trials take 5.2 ms, 256k 7.0 ms (1.27e7 vs 3.74e7 trials/s,
    // profiles/r2p_abc_batch_sweep.jsonl), so a smaller batch saves nothing and a second launch costs a whole floor.
    const int64_t cap_days = ((int64_t)1 << 32) / (12 * (int64_t)T);
    const int max_batch = (int)std::max<int64_t>(256, std::min<int64_t>(batch > 0 ? batch : (1 << 20), cap_days));
    const int min_batch = std::min(1 << 18, max_batch);
    int cur = batch > 0 ? std::min(batch, max_batch) : min_batch;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = abc_buffers(c, T, max_batch, no_of_samples, p, n_prev)) return rc;
    AbcArgs a = p.args;
    AbcSmcArgs m{};
    if (n_prev > 0) {
        m.prev_theta = p.prev_theta; m.cdf = p.prev_cdf; m.n_prev = n_prev; m.anc = p.anc;
        for (int q = 0; q < 2; ++q) { m.half[q] = prev.half_width[q]; m.hi[q] = priors[2 * q + 1]; }
        HIP_TRY(hipMemcpyAsync(p.prev_theta, prev.theta, sizeof(double) * 2 * (size_t)n_prev, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p.prev_cdf, prev.cdf, sizeof(double) * (size_t)n_prev, hipMemcpyHostToDevice, c->stream));
    }
    // Early rejection: the device distance is fl(fl(fl(si/T) + fl(sr/T))/2) with si, sr numpy-pairwise
    // sums of the non-negative terms fl(|x_d - y_d|), so it is at least the exact (sum_I + sum_R)/(2T) times
    // (1-u)^(T+4), and a lane's running sum `acc` of the same terms is at most that exact sum times (1+u)^(2T+2)
    // (u = 2^-53).  acc > 2T threshold (1 + 1e-9) therefore proves distance > threshold (for T <= kAbcMaxDays,
    // (3T+8)u < 2e-10), i.e. the trial is rejected (abc_algo.py:30-33).  Only for a threshold well inside the normal
    // range (no subnormal quotients); EPIPF_ABC_EARLY=0 turns it off (the results are identical either way).
    bool early = threshold >= 1e-200 && threshold <= 1e200;
    if (const char* e = getenv("EPIPF_ABC_EARLY")) early = early && atoi(e) != 0;
    if (early) a.reject_sum = 2.0 * (double)T * threshold * (1.0 + 1e-9);
    HIP_TRY(hipMemcpyAsync(p.Ydev, Y, sizeof(double) * 3 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    int have = 0;
    int64_t t = 0, last = -1;
    int32_t* h_cnt = c->h_status;   // pinned staging (>= 1 entry)
    while (have < no_of_samples && t < max_trials) {
        const int nb = (int)std::min<int64_t>(cur, max_trials - t);
        if (n_prev > 0) {
            if (int rc = abc_launch_smc_trials(c, a, m, (uint32_t)(t0 + t), nb)) return rc;
        } else {
            if (int rc = abc_launch_trials(c, a, (uint32_t)(t0 + t), nb)) return rc;
        }
        AbcSelectArgs s{};
        s.dist = a.dist; s.n = nb; s.need = no_of_samples - have; s.threshold = threshold; s.idx = p.idx; s.count = p.count;
        hipError_t le = launch_abc_select(s, c->stream);
        if (le != hipSuccess) return fail(EPIPF_EHIP, "ABC select launch failed: %s", hipGetErrorString(le));
        AbcGatherArgs g{};
        g.days = a.days; g.theta = a.theta; g.idx = p.idx; g.count = p.count; g.n = nb; g.T = T; g.slot0 = have;
        g.traj = p.traj; g.theta_out = p.theta_out;
        g.dist = a.dist; g.anc = n_prev > 0 ? p.anc : nullptr; g.dist_out = p.dist_out; g.anc_out = p.anc_out;
        le = launch_abc_gather(g, no_of_samples - have, c->stream);
        if (le != hipSuccess) return fail(EPIPF_EHIP, "ABC gather launch failed: %s", hipGetErrorString(le));
        HIP_TRY(hipMemcpyAsync(h_cnt, p.count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = abc_account(c, nb)) return rc;
        const int got = h_cnt[0];
        if (got > 0) {
            HIP_TRY(hipMemcpyAsync(h_cnt, p.idx + got - 1, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            last = t + h_cnt[0];
        }
        have += got;
        t += nb;
        if (batch <= 0) {
            const double want = have > 0 ? 1.25 * (double)(no_of_samples - have) * (double)t / (double)have
                                              : 4.0 * cur;
            cur = (int)std::max<double>(std::min<double>(want + 1024.0, (double)max_batch), (double)min_batch);
        }
    }
    if (have > 0) {
        HIP_TRY(hipMemcpyAsync(theta_out, p.theta_out, sizeof(double) * 2 * (size_t)have, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(traj_out, p.traj, sizeof(double) * 4 * (size_t)T * have, hipMemcpyDeviceToHost, c->stream));
        if (dist_out)
            HIP_TRY(hipMemcpyAsync(dist_out, p.dist_out, sizeof(double) * (size_t)have, hipMemcpyDeviceToHost, c->stream));
        if (ancestor_out)
            HIP_TRY(hipMemcpyAsync(ancestor_out, p.anc_out, sizeof(int32_t) * (size_t)have, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (int rc = abc_read_counters(c)) return rc;
    *accepted_out = have;
    *trials_out = have == no_of_samples ? last + 1 : t;
    return EPIPF_OK;
}
}  // namespace

int epipf_abc(epipf_ctx* c, const double* Y, int T, int no_of_samples, double threshold, const double* priors,
              uint64_t key, uint32_t run_index, int64_t max_trials, int batch, double* theta_out, double* traj_out,
              int64_t* trials_out, int32_t* accepted_out) {
    return abc_sample(c, Y, T, no_of_samples, threshold, priors, AbcSmcPrev{nullptr, nullptr, 0, nullptr}, key,
                      run_index, 0u, max_trials, batch, theta_out, traj_out, nullptr, nullptr, trials_out, accepted_out);
}

int epipf_abc_smc_generation(epipf_ctx* c, const double* Y, int T, int no_of_samples, double threshold,
                             const double* priors, const double* prev_theta, const double* prev_cdf, int n_prev,
                             const double* half_width, uint64_t key, uint32_t run_index, uint32_t t0,
                             int64_t max_trials, int batch, double* theta_out, double* traj_out, double* dist_out,
                             int32_t* ancestor_out, int64_t* trials_out, int32_t* accepted_out) {
    if (n_prev < 0) return fail(EPIPF_EINVAL, "n_prev < 0");
    if (!dist_out || !ancestor_out) return fail(EPIPF_EINVAL, "NULL output pointer");
    return abc_sample(c, Y, T, no_of_samples, threshold, priors, AbcSmcPrev{prev_theta, prev_cdf, n_prev, half_width},
                      key, run_index, t0, max_trials, batch, theta_out, traj_out, dist_out, ancestor_out, trials_out,
                      accepted_out);
}

int epipf_abc_smc_weights(epipf_ctx* c, const double* theta, int n, const double* prev_theta, const double* prev_w,
                          int n_prev, const double* half_width, double* den_out) {
    if (!c || !theta || !prev_theta || !prev_w || !half_width || !den_out) return fail(EPIPF_EINVAL, "NULL argument");
    if (n < 0 || n_prev < 1) return fail(EPIPF_EINVAL, "n=%d, n_prev=%d: need n >= 0 and n_prev >= 1", n, n_prev);
    for (int q = 0; q < 2; ++q)
        if (!(half_width[q] >= 0.0 && half_width[q] < INFINITY))
            return fail(EPIPF_EINVAL, "half_width[%d]=%g: kernel half-widths must be finite and >= 0", q, half_width[q]);
    for (int q = 0; q < n_prev; ++q)
        if (!(prev_w[q] >= 0.0 && prev_w[q] < INFINITY))
            return fail(EPIPF_EINVAL, "prev_w[%d]=%g: weights must be finite and >= 0", q, prev_w[q]);
    if (n == 0) return EPIPF_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t sz_t = align256(sizeof(double) * 2 * (size_t)n), sz_pt = align256(sizeof(double) * 2 * (size_t)n_prev),
                 sz_w = align256(sizeof(double) * (size_t)n_prev), sz_d = align256(sizeof(double) * (size_t)n);
    char* buf = nullptr;
    if (hipMalloc((void**)&buf, sz_t + sz_pt + sz_w + sz_d) != hipSuccess)
        return fail(EPIPF_ENOMEM, "ABC-SMC weight buffers hipMalloc(%zu) failed", sz_t + sz_pt + sz_w + sz_d);
    AbcSmcWeightArgs a{};
    a.theta = (double*)buf;
    a.prev_theta = (double*)(buf + sz_t);
    a.prev_w = (double*)(buf + sz_t + sz_pt);
    a.den = (double*)(buf + sz_t + sz_pt + sz_w);
    a.n = n;
    a.n_prev = n_prev;
    a.half[0] = half_width[0];
    a.half[1] = half_width[1];
    hipError_t e = hipMemcpyAsync((void*)a.theta, theta, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync((void*)a.prev_theta, prev_theta, sizeof(double) * 2 * (size_t)n_prev, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync((void*)a.prev_w, prev_w, sizeof(double) * (size_t)n_prev, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_abc_smc_weights(a, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(den_out, a.den, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(EPIPF_EHIP, "ABC-SMC weights: %s", hipGetErrorString(e));
    return EPIPF_OK;
}

int epipf_set_profiling(epipf_ctx* c, int enable) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (enable < EPIPF_PROFILE_OFF || enable > EPIPF_PROFILE_COUNTERS) return fail(EPIPF_EINVAL, "bad profiling level %d", enable);
    c->profiling = enable;
    return EPIPF_OK;
}

int epipf_set_streams(epipf_ctx* c, int n_streams) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (n_streams < 1 || n_streams > kMaxFilterStreams)
        return fail(EPIPF_EINVAL, "n_streams %d outside [1, %d]", n_streams, kMaxFilterStreams);
    c->n_streams = n_streams;     // streams are created at the first run that uses them
    return EPIPF_OK;
}

int epipf_set_lanes(epipf_ctx* c, int lanes, int events_per_lane) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    if (!(lanes == 0 || lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16))
        return fail(EPIPF_EINVAL, "lanes %d not in {0 (automatic), 1, 2, 4, 8, 16}", lanes);
    if (events_per_lane < 0) return fail(EPIPF_EINVAL, "events_per_lane %d < 0", events_per_lane);
    if (lanes > 1 && events_per_lane > 0 && !group_shape_supported(lanes, events_per_lane))
        return fail(EPIPF_EINVAL, "no lane-group kernel for %d lanes x %d events per lane", lanes, events_per_lane);
    if (lanes > 1 && c->G > kMaxLaneG)
        return fail(EPIPF_EINVAL, "%d lanes per particle with G=%d: lane groups exist for G <= %d", lanes, c->G, kMaxLaneG);
    c->lanes = lanes;
    c->lane_events = events_per_lane;
    return EPIPF_OK;
}

int epipf_get_stats(epipf_ctx* c, epipf_stats* out) {
    if (!c || !out) return fail(EPIPF_EINVAL, "NULL argument");
    *out = c->stats;
    return EPIPF_OK;
}

int epipf_reset_stats(epipf_ctx* c) {
    if (!c) return fail(EPIPF_EINVAL, "NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * (size_t)kCounterSlots * kCounterStride, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(&c->stats, 0, sizeof c->stats);
    return EPIPF_OK;
}

}  // extern "C"
