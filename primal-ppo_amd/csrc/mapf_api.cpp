// primal-ppo_amd/csrc/mapf_api.cpp -- the C ABI (include/mapf.h) over the HIP kernels.
//
// Host responsibilities: validate configs and reset inputs (the reference
// raises Python exceptions where this returns MAPF_EINVAL), own the device
// SoA state, build the padded obstacle bitmaps and the fp64-derived lookup
// tables, and order the kernels of one step on the caller's stream:
//   step_kernel -> replan_kernel (human paths, if the human can replan)
//               -> bfs_kernel (agent.bfsMap on goal changes, if keep_bfs)
// No allocation, copy or synchronisation happens inside mapf_step /
// mapf_observe, so both can be captured into a hipGraph by the caller.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mapf.h"
#include "mapf_kernels.h"
#include "mapf_group.h"     // pace_gate, evaluated on the host by mapf_pace_gate
#include "mapf_observe.h"  // obs_band_skip, evaluated on the host by mapf_obs_band_skip
#include "mapf_obs_bits.h"
#include "mapf_sym.h"      // the grid symmetries, evaluated on the host by mapf_sym_*

using namespace mapf;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t _e = (x);                                                                       \
        if (_e != hipSuccess) return fail(MAPF_EDEVICE, std::string(#x) + ": " + hipGetErrorString(_e)); \
    } while (0)

int next_pow2(int n) {
    int g = 1;
    while (g < n) g <<= 1;
    return g;
}
}  // namespace

struct mapf_env {
    mapf_config cfg;
    int device = 0;
    DevEnv d{};
    int parity = 1;          // work-list slot of the next step (step count mod 3)
    int pending = -1;        // slot whose search work has not been launched yet
    bool ready = false;
    std::vector<void *> allocs;
    int8_t *maps8 = nullptr;  // [nmaps][H][W] int8 maps on the device (uploaded or generated)
    // second stream for a search that runs beside the observe launch (fork/join inside
    // one API call, so the caller's stream -- and a hipGraph capture of it -- sees one
    // sequence); created on first use
    hipStream_t aux = nullptr, aux2 = nullptr;   // aux: BFS maps the observation reads; aux2: deferred work
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    // Deferred joins.  A human's next path is read no earlier than two steps after its
    // step queued it (mapf_fused.hip), and agent BFS maps only by the BFS channel
    // (C = 7, joined at once) and mapf_bfs: so the aux-stream search of committed step t
    // runs beside step t+1 and is joined on the caller's stream before step t+2 -- or
    // before anything else reads or rewrites the state (join_deferred).
    long nsteps = 0;                       // committed steps since the reset
    hipEvent_t ev_def[2] = {nullptr, nullptr};
    long def_due[2] = {-1, -1};            // join before the step that would make nsteps exceed this
    int def_next = 0;
    mapf_tuning tune;                      // launch forms (mapf_set_tuning); never the process environment
    int max_lds = 0;                       // device_max_group_lds() of `device`: what the observe launch is fitted to
    ArgRing args;                          // device-resident argument blocks of the persistent kernels
    // the PIBT policy's age arrays [B][N] (mapf.h: mapf_pibt_actions): the packed goal last seen and
    // the clock it was first seen at; policy-owned, no step kernel touches them
    uint32_t *pibt_seen = nullptr, *pibt_since = nullptr;
    // mapf_rollout_perf's per-step route: one step's outputs [B][N] (perf_accumulate reads them) and the
    // [B][N] actions of a step where the caller takes none (mapf_step needs them).  Only on handles the
    // one-wave-per-env kernel does not cover: every other handle has a perf kernel for every policy,
    // and those store no action the caller did not ask for.
    int32_t *perf_act = nullptr;
    mapf_step_out perf_step{};
    // mapf_set_action_noise's per-step route: the [B][N] row of played actions the step runs from (the
    // policy's pick, the label, stays in the caller's row, or in perf_act where the caller takes none)
    int32_t *noise_act = nullptr;
    int pibt_horizon = 1;     // the PIBT policy's human horizon K (mapf_set_pibt_human_horizon); in d.pibt_w while the weight is above 0
    template <class T>
    int alloc(T *&p, size_t n) {
        void *q = nullptr;
        if (n == 0) n = 1;
        if (hipMalloc(&q, n * sizeof(T)) != hipSuccess) return fail(MAPF_ENOMEM, "hipMalloc failed");
        allocs.push_back(q);
        p = reinterpret_cast<T *>(q);
        return 0;
    }
};

// what mapf_create checks before any device call
static int check_config(const mapf_config &c) {
    if (c.num_envs < 1) return fail(MAPF_EINVAL, "num_envs must be >= 1");
    if (c.num_agents < 1 || c.num_agents > 64) return fail(MAPF_EINVAL, "num_agents must be in 1..64");
    if (c.height < 1 || c.height > 128 || c.width < 1 || c.width > 128) return fail(MAPF_EINVAL, "height/width must be in 1..128");
    if (c.fov < 1 || c.fov > 16) return fail(MAPF_EINVAL, "fov must be in 1..16");
    if (c.num_channel < 5 || c.num_channel > 7) return fail(MAPF_EINVAL, "num_channel must be 5, 6 or 7");
    if (c.num_channel == 7 && !c.keep_bfs) return fail(MAPF_EINVAL, "num_channel 7 (BFS channel) needs keep_bfs");
    if (c.human_mode < 0 || c.human_mode > 2) return fail(MAPF_EINVAL, "human_mode must be 0, 1 or 2");
    if (c.goal_mode < 0 || c.goal_mode > 1) return fail(MAPF_EINVAL, "goal_mode must be 0 or 1");
    if (c.fix_choice < 0 || c.fix_choice > 1) return fail(MAPF_EINVAL, "fix_choice must be 0 or 1");
    if (c.max_seq < 1) return fail(MAPF_EINVAL, "max_seq must be >= 1");
    if (c.human_mode == 2 && c.max_human_seq < 2) return fail(MAPF_EINVAL, "max_human_seq must be >= 2");
    if (c.penalty_radius < 1 || c.penalty_radius > 64) return fail(MAPF_EINVAL, "penalty_radius must be in 1..64");
    if (c.k_predict < 0 || c.k_predict > 64) return fail(MAPF_EINVAL, "k_predict must be in 0..64");
    return MAPF_OK;
}

// the sizes and switches of a checked config, as the kernels read them (no pointers, no tuning)
static void config_geometry(const mapf_config &c, DevEnv &d) {
    d.B = c.num_envs; d.N = c.num_agents; d.H = c.height; d.W = c.width; d.F = c.fov; d.C = c.num_channel;
    d.P = c.fov / 2 > 1 ? c.fov / 2 : 1;
    d.Hp = d.H + 2 * d.P;
    d.WW = (d.W + 2 * d.P + 31) / 32;
    d.G = next_pow2(d.N);
    d.S = c.max_seq;
    d.HS = c.max_human_seq > 2 ? c.max_human_seq : 2;
    d.Lmax = 2 * d.H * d.W + 1;
    d.use_da = c.use_da; d.use_hp = c.use_hp; d.lifelong = c.lifelong; d.human_mode = c.human_mode;
    d.goal_mode = c.goal_mode; d.fix_choice = c.fix_choice; d.shared_map = c.shared_map ? 1 : 0;
    d.keep_bfs = c.keep_bfs ? 1 : 0; d.k_predict = c.k_predict; d.R = c.penalty_radius;
    d.action_cost = c.action_cost; d.collision_cost = c.collision_cost; d.human_collision_cost = c.human_collision_cost;
    d.repeat_cost = c.repeat_cost; d.goal_reward = c.goal_reward;
    d.env_offset = (uint32_t)c.env_offset;
    d.seed = c.seed;
}

// Envs per observe_kernel workgroup for the tuning value obs_envs.  `want`: that value, or for 0 the
// default rule (64/N fills a wave's lanes for N <= 8; above that one env per workgroup measured
// fastest -- c4, 16 agents: 12.4 us vs 14.2 us at 4 envs, tools/sweep_c45.sh), at most B.  Returns the
// largest count <= want whose launch fits max_lds bytes of LDS (0: not even one env does): the index
// image alone is H*W bytes per env, so few agents on a large map do not fit at 64/N.
static int observe_envs(const DevEnv &d, int obs_envs, size_t max_lds, int &want) {
    want = obs_envs > 0 ? std::min(obs_envs, d.B) : observe_default_envs(d);
    return observe_fit_envs(d, want, max_lds);
}

// the per-step launches' tuning fields live in DevEnv (the kernels read them); obs_envs as observe_envs fitted it
static void apply_tuning(DevEnv &d, const mapf_tuning &t, int obs_envs) {
    d.obs_envs = obs_envs;
    d.step_block = t.step_block;
    d.search_blocks = t.search_blocks;
    d.band_blocks = t.band_blocks;   // zero-band workgroups: slower than the waves' table-driven stores (0)
    d.force_agent_lanes = t.agent_lanes;
}

// DevEnv::constr_d2: the largest d2 with (R - sqrt(d2)) / R >= 0.01 in fp64 (monotone in d2, mapf_gym.py:633)
static int constr_d2_of(int radius) {
    const double R = (double)radius;
    int best = -1;
    for (int k = 0; k <= radius * radius; ++k) {
        double v = R - std::sqrt((double)k);
        if (!(v > 0.0)) v = 0.0;
        if (v / R >= 0.01) best = k;
    }
    return best;
}

extern "C" {

void mapf_tuning_default(mapf_tuning *t) {
    if (!t) return;
    *t = mapf_tuning{};
    t->roll_occ = 0;
    t->roll_group = -1;
    t->roll_fair = -1;
    t->roll_slack = 1;
    t->wide_nt = -1;
    t->wide_pipe = 1;
    t->wide_grid = 1;
    t->wide_overlap = 1;
    t->wide_obs = 2;
    t->wide_epw = 0;
    t->wide_pair = 0;
    t->wide_slack = 1;
    t->wide_fair = 0;
    t->wide_prio = 1;
    t->wide_bfsobs = 1;
    t->xcd_remap = 1;
    t->obs_envs = 0;
    t->step_block = 256;
    t->search_blocks = 64;
    t->band_blocks = 0;
    t->agent_lanes = 0;
    t->serial_search = 0;
    t->no_defer = 0;
    t->diag_exp = 0;
}

int mapf_get_tuning(const mapf_env *e, mapf_tuning *t) {
    if (!e || !t) return fail(MAPF_EINVAL, "null argument");
    *t = e->tune;
    return MAPF_OK;
}

int mapf_set_tuning(mapf_env *e, const mapf_tuning *t) {
    if (!e || !t) return fail(MAPF_EINVAL, "null argument");
    auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
    auto flag = [&](int v) { return in(v, 0, 1); };
    if (!in(t->roll_occ, 0, 16)) return fail(MAPF_EINVAL, "roll_occ must be in 0..16");
    if (!in(t->roll_group, -1, 1)) return fail(MAPF_EINVAL, "roll_group must be -1, 0 or 1");
    if (!in(t->roll_fair, -1, 1 << 20)) return fail(MAPF_EINVAL, "roll_fair must be >= -1");
    if (!in(t->roll_slack, -1, 1 << 20)) return fail(MAPF_EINVAL, "roll_slack must be >= -1");
    if (!in(t->wide_nt, -1, 1)) return fail(MAPF_EINVAL, "wide_nt must be -1, 0 or 1");
    if (!flag(t->wide_pipe) || !flag(t->wide_grid) || !flag(t->wide_overlap) || !flag(t->wide_pair) ||
        !flag(t->wide_prio) || !flag(t->wide_bfsobs) || !flag(t->xcd_remap) || !flag(t->agent_lanes) ||
        !flag(t->serial_search) || !flag(t->no_defer))
        return fail(MAPF_EINVAL, "wide_pipe/grid/overlap/pair/prio/bfsobs, xcd_remap, agent_lanes, serial_search, "
                                 "no_defer must be 0 or 1");
    if (!in(t->wide_obs, 1, 2)) return fail(MAPF_EINVAL, "wide_obs must be 1 or 2");
    if (!in(t->wide_epw, 0, 12)) return fail(MAPF_EINVAL, "wide_epw must be in 0..12");
    if (!in(t->wide_slack, -1, 1 << 20)) return fail(MAPF_EINVAL, "wide_slack must be >= -1");
    if (!in(t->wide_fair, 0, 1 << 20)) return fail(MAPF_EINVAL, "wide_fair must be >= 0");
    if (!in(t->obs_envs, 0, 64)) return fail(MAPF_EINVAL, "obs_envs must be in 0..64");
    if (t->step_block != 64 && t->step_block != 128 && t->step_block != 256)
        return fail(MAPF_EINVAL, "step_block must be 64, 128 or 256");
    if (!in(t->search_blocks, 1, 1024)) return fail(MAPF_EINVAL, "search_blocks must be in 1..1024");
    if (!in(t->band_blocks, 0, 4096)) return fail(MAPF_EINVAL, "band_blocks must be in 0..4096");
    if (!in(t->diag_exp, 0, 3)) return fail(MAPF_EINVAL, "diag_exp must be in 0..3");
    int want = 0;
    const int envs = observe_envs(e->d, t->obs_envs, (size_t)e->max_lds, want);
    if (t->obs_envs > 0 && envs != want)      // (the default, 0, is reduced instead: mapf_create saw one env fit)
        return fail(MAPF_EINVAL, "obs_envs " + std::to_string(want) + " needs " +
                                     std::to_string(observe_launch_lds(e->d, want)) + " bytes of LDS per observe workgroup, "
                                     "over the device's " + std::to_string(e->max_lds) + ": the largest value that fits is " +
                                     std::to_string(envs));
    e->tune = *t;
    apply_tuning(e->d, e->tune, envs);
    return MAPF_OK;
}

const char *mapf_last_error(void) { return g_err.c_str(); }
int mapf_abi_version(void) { return MAPF_ABI_VERSION; }

int mapf_create(const mapf_config *cfg, int device, mapf_env **out) {
    if (!cfg || !out) return fail(MAPF_EINVAL, "null argument");
    const mapf_config &c = *cfg;
    if (int rc = check_config(c)) return rc;
    if (hipSetDevice(device) != hipSuccess) return fail(MAPF_EDEVICE, "hipSetDevice failed");

    auto *e = new mapf_env();
    e->cfg = c;
    e->device = device;
    DevEnv &d = e->d;
    config_geometry(c, d);
    mapf_tuning_default(&e->tune);
    e->max_lds = device_max_group_lds();
    int want = 0;
    const int envs = observe_envs(d, e->tune.obs_envs, (size_t)e->max_lds, want);
    if (envs < 1) {     // refused here, not by the first observe launch
        const size_t need = observe_launch_lds(d, 1);
        delete e;
        return fail(MAPF_EINVAL, "one env's observe workgroup needs " + std::to_string(need) + " bytes of LDS, over the device's " +
                                     std::to_string(device_max_group_lds()));
    }
    apply_tuning(d, e->tune, envs);
    d.pibt_w = 0;       // the PIBT policy is blind to the safety radius until mapf_set_pibt_human_weight

    // fp64 lookup table, computed exactly like the reference (numpy sqrt)
    const double R = (double)c.penalty_radius;
    std::vector<float> cost_lut(d.R * d.R + 1);
    d.constr_d2 = constr_d2_of(c.penalty_radius);
    for (int k = 0; k <= d.R * d.R; ++k) {
        double v = R - std::sqrt((double)k);      // np.linalg.norm -> sqrt (mapf_gym.py:519)
        if (!(v > 0.0)) v = 0.0;
        cost_lut[k] = (float)(v / R);
    }

    const size_t BN = (size_t)d.B * d.N;
    const size_t nmaps = d.shared_map ? 1 : (size_t)d.B;
    int rc = 0;
    uint32_t *map_bits = nullptr;
    float *cl = nullptr;
    rc |= e->alloc(map_bits, nmaps * d.Hp * d.WW);
    rc |= e->alloc(d.pos, BN); rc |= e->alloc(d.goal, BN); rc |= e->alloc(d.last_act, BN);
    rc |= e->alloc(d.seq, BN * d.S); rc |= e->alloc(d.seq_len, BN); rc |= e->alloc(d.seq_cur, BN);
    rc |= e->alloc(d.hpath, (size_t)d.B * 2 * d.Lmax);
    rc |= e->alloc(d.hlen, 2 * (size_t)d.B); rc |= e->alloc(d.hstep, d.B); rc |= e->alloc(d.hcur, d.B);
    rc |= e->alloc(d.hpos, d.B); rc |= e->alloc(d.hnext, d.B); rc |= e->alloc(d.hgoal, d.B); rc |= e->alloc(d.hentr, d.B);
    rc |= e->alloc(d.hnext_start, d.B); rc |= e->alloc(d.hnext_goal, d.B);
    rc |= e->alloc(d.hseq, (size_t)d.B * d.HS); rc |= e->alloc(d.hseq_len, d.B); rc |= e->alloc(d.hseq_idx, d.B);
    rc |= e->alloc(d.hreplans, d.B); rc |= e->alloc(d.clock, d.B);
    if (d.keep_bfs) rc |= e->alloc(d.bfs, BN * bfs_cells(d.H, d.W));
    rc |= e->alloc(d.counters, C_NUM);
    rc |= e->alloc(d.prof, PROF_WORDS);
    rc |= e->alloc(d.replan_list, 3 * (size_t)d.B);
    rc |= e->alloc(d.bfs_list, 3 * BN);
    uint8_t *smask = nullptr;
    rc |= e->alloc(smask, nmaps * (size_t)d.H * d.W);
    rc |= e->alloc(e->maps8, nmaps * (size_t)d.H * d.W);
    rc |= e->alloc(cl, cost_lut.size());
    rc |= e->alloc(e->args.base, (ARG_SLOTS + ARG_CAPTURE_SLOTS) * ARG_SLOT_BYTES);
    rc |= e->alloc(e->pibt_seen, BN); rc |= e->alloc(e->pibt_since, BN);
    rc |= e->alloc(e->noise_act, BN);
    if (!rollout_wide_fusable(d)) {
        mapf_step_out &ps = e->perf_step;
        rc |= e->alloc(e->perf_act, BN);
        rc |= e->alloc(ps.status, BN); rc |= e->alloc(ps.reward_total, BN); rc |= e->alloc(ps.cost, BN);
        rc |= e->alloc(ps.goals_reached, BN); rc |= e->alloc(ps.constraints, BN);
        rc |= e->alloc(ps.shadow_goals, (size_t)d.B);
    }
    if (rc) {
        std::string m = g_err;
        mapf_destroy(e);
        return fail(MAPF_ENOMEM, m);
    }
    d.map_bits = map_bits;
    d.smask = smask;
    d.cost_lut = cl;
    if (hipMemcpy(cl, cost_lut.data(), cost_lut.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d.counters, 0, C_NUM * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(d.prof, 0, PROF_WORDS * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(e->pibt_seen, 0, BN * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(e->pibt_since, 0xFF, BN * sizeof(uint32_t)) != hipSuccess) {
        mapf_destroy(e);
        return fail(MAPF_EDEVICE, "initial upload failed");
    }
    *out = e;
    return MAPF_OK;
}

int mapf_destroy(mapf_env *e) {
    if (!e) return MAPF_OK;
    (void)hipSetDevice(e->device);
    if (e->aux) {
        (void)hipStreamSynchronize(e->aux);
        (void)hipStreamDestroy(e->aux);
    }
    if (e->aux2) {
        (void)hipStreamSynchronize(e->aux2);
        (void)hipStreamDestroy(e->aux2);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->ev_join2) (void)hipEventDestroy(e->ev_join2);
    for (hipEvent_t ev : e->ev_def)
        if (ev) (void)hipEventDestroy(ev);
    for (void *p : e->allocs) (void)hipFree(p);
    delete e;
    return MAPF_OK;
}

int mapf_path_capacity(const mapf_env *e) { return e ? e->d.Lmax : 0; }
int mapf_step_observe_fused(const mapf_env *e) { return e && step_observe_fusable(e->d) ? 1 : 0; }
static int check_policy(int policy) {
    if (policy < ROLLOUT_RANDOM || policy > ROLLOUT_PIBT) return fail(MAPF_EINVAL, "policy must be 0..3");
    return MAPF_OK;
}
// descent and PIBT pick from the agents' tiled BFS maps
static bool needs_bfs(int policy) { return policy == ROLLOUT_DESCENT || policy == ROLLOUT_PIBT; }

// what a *_plan call knows of the rollout call it describes
static RolloutReq plan_req(RolloutForm form, int policy, int slots, const float *obs = nullptr) {
    RolloutReq q{};
    q.form = form;
    q.policy = policy;
    q.slots = slots;
    q.obs = const_cast<float *>(obs);
    return q;
}

int mapf_rollout_random_fused(const mapf_env *e) { return e ? rollout_route(e->d, plan_req(ROLLOUT_OBSERVE, ROLLOUT_RANDOM, 0)) : 0; }

// the PIBT weight / horizon after a plan's text: run-time values of the same kernel, so trailing words
static void pibt_plan_suffix(const mapf_env *e, char *buf, int32_t n) {
    if (e->d.pibt_w == 0) return;
    const size_t len = std::strlen(buf);
    if (e->pibt_horizon > 1)
        std::snprintf(buf + len, (size_t)n - len, " human_weight=%d human_horizon=%d", pibt_w_weight(e->d.pibt_w),
                      e->pibt_horizon);
    else
        std::snprintf(buf + len, (size_t)n - len, " human_weight=%d", pibt_w_weight(e->d.pibt_w));
}

// Every *_plan call: the request's route as the kind, and as text the kernel's form there or the per-step
// launches -- the switch rollout_run makes
static int rollout_plan(const mapf_env *e, const RolloutReq &q, char *buf, int32_t n) {
    if (!e || !buf || n < 1) return fail(MAPF_EINVAL, "null argument");
    if (int rc = check_policy(q.policy)) return rc;
    if (hipSetDevice(e->device) != hipSuccess) return fail(MAPF_EDEVICE, "hipSetDevice failed");
    const bool perf = q.form == ROLLOUT_PERF;
    const int route = rollout_route(e->d, q);
    switch (route) {
        case ROUTE_PAIRS: (perf ? describe_rollout_perf : describe_rollout_random)(e->d, q, e->tune, buf, (size_t)n); break;
        case ROUTE_WIDE: (perf ? describe_rollout_wide_perf : describe_rollout_wide)(e->d, q, e->tune, buf, (size_t)n); break;
        default:
            std::snprintf(buf, (size_t)n, "%sstep%s",
                          q.policy == ROLLOUT_PIBT ? "pibt_actions+" : (q.policy == ROLLOUT_DESCENT ? "descent_actions+" : ""),
                          perf ? "+perf_accumulate" : ((q.slots & MAPF_SLOTS_OBS_BITS) ? "_observe_bits" : "_observe"));
    }
    if (q.policy == ROLLOUT_PIBT && q.form != ROLLOUT_SPARSE) pibt_plan_suffix(e, buf, n);   // (the sparse plan carries none)
    if (needs_bfs(q.policy) && e->d.noise_q16 > 0) {       // the threshold of the ",noise" instantiation: after the PIBT words
        const size_t len = std::strlen(buf);
        std::snprintf(buf + len, (size_t)n - len, " noise=%d", e->d.noise_q16);
    }
    return route;
}
int mapf_rollout_plan(const mapf_env *e, int32_t slots, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_OBSERVE, ROLLOUT_RANDOM, slots), buf, n);
}
int mapf_rollout_actions_plan(const mapf_env *e, int32_t slots, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_OBSERVE, ROLLOUT_TAPE, slots), buf, n);
}
int mapf_rollout_descent_plan(const mapf_env *e, int32_t slots, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_OBSERVE, ROLLOUT_DESCENT, slots), buf, n);
}
int mapf_rollout_pibt_plan(const mapf_env *e, int32_t slots, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_OBSERVE, ROLLOUT_PIBT, slots), buf, n);
}
// (a shadow that describes every slot: the band-clean launch where the sparse form does not apply)
int mapf_rollout_sparse_plan(const mapf_env *e, int32_t policy, const float *obs, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_SPARSE, policy, MAPF_SLOTS | MAPF_SLOTS_BAND_CLEAN, obs), buf, n);
}
int mapf_rollout_perf_plan(const mapf_env *e, int32_t policy, char *buf, int32_t n) {
    return rollout_plan(e, plan_req(ROLLOUT_PERF, policy, 0), buf, n);
}

int mapf_descent_pick(uint32_t descent_mask, uint32_t clock, int32_t agent) {
    return descent_pick(descent_mask, clock, (int)agent);
}

int mapf_pibt_key(int32_t dist, int32_t action, uint32_t clock, int32_t agent) {
    return pibt_key((int)dist, (int)action, clock, (int)agent);
}

int mapf_pibt_human_level(int32_t penalty_radius, int32_t d2) {
    if (penalty_radius < 1 || penalty_radius > 64) return fail(MAPF_EINVAL, "penalty_radius must be in 1..64");
    if (d2 < 0) return fail(MAPF_EINVAL, "d2 must be >= 0");
    return pibt_human_level((int)penalty_radius, constr_d2_of((int)penalty_radius), (int)d2);
}

int mapf_set_action_noise(mapf_env *e, int32_t noise_q16) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    if (noise_q16 < 0 || noise_q16 > 65536) return fail(MAPF_EINVAL, "the action noise must be in 0..65536");
    e->d.noise_q16 = (int)noise_q16;      // a kernel argument of the next launch: no device call
    return MAPF_OK;
}

int mapf_get_action_noise(const mapf_env *e) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    return e->d.noise_q16;
}

int mapf_action_noise_pick(uint64_t seed, uint32_t env_id, int32_t agent, uint32_t clock, int32_t noise_q16,
                           int32_t label) {
    if (agent < 0 || agent > 63) return fail(MAPF_EINVAL, "agent must be in 0..63");
    if (label < 0 || label >= NA) return fail(MAPF_EINVAL, "label must be in 0..4");
    if (noise_q16 < 0 || noise_q16 > 65536) return fail(MAPF_EINVAL, "the action noise must be in 0..65536");
    if (noise_q16 == 0) return label;     // the kernels' branch: no draw
    return action_noise_pick(seed, env_id, (int)agent, clock, (int)noise_q16, (int)label);
}

int mapf_set_pibt_human_weight(mapf_env *e, int32_t weight) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    if (weight < 0 || weight > 16) return fail(MAPF_EINVAL, "the PIBT human weight must be in 0..16");
    // a kernel argument of the next pick or rollout launch: no device call
    e->d.pibt_w = pibt_w_pack((int)weight, e->d.R, e->d.constr_d2, e->pibt_horizon);
    return MAPF_OK;
}

int mapf_set_pibt_human_horizon(mapf_env *e, int32_t k) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    if (k < 1 || k > PIBT_HORIZON_MAX) return fail(MAPF_EINVAL, "the PIBT human horizon must be in 1..8");
    // kept on the handle (at weight 0 the kernels' word is 0 whatever the horizon) and in the word: no device call
    e->pibt_horizon = (int)k;
    e->d.pibt_w = pibt_w_pack(pibt_w_weight(e->d.pibt_w), e->d.R, e->d.constr_d2, e->pibt_horizon);
    return MAPF_OK;
}

int mapf_get_pibt_human_horizon(const mapf_env *e) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    return e->pibt_horizon;
}

int mapf_pibt_w_word(int32_t weight, int32_t penalty_radius, int32_t constr_d2, int32_t k, int32_t *fields) {
    if (weight < 0 || weight > 16 || penalty_radius < 1 || penalty_radius > 64 || constr_d2 < 0 || constr_d2 > 4095 ||
        k < 1 || k > PIBT_HORIZON_MAX) {
        fail(MAPF_EINVAL, "mapf_pibt_w_word: a field out of range");
        return -1;
    }
    const int word = pibt_w_pack((int)weight, (int)penalty_radius, (int)constr_d2, (int)k);
    if (fields) {
        fields[0] = pibt_w_weight(word);
        fields[1] = pibt_w_radius(word);
        fields[2] = pibt_w_constr_d2(word);
        fields[3] = pibt_w_horizon(word);
    }
    return word;
}

int mapf_get_pibt_human_weight(const mapf_env *e) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    return pibt_w_weight(e->d.pibt_w);
}

// Step 3 of the policy (mapf.h: mapf_pibt_actions), sequentially: the recursion as the chain of
// parent indices the wave form keeps one per lane (mapf_pibt.h: pibt_solve_wave).
int mapf_pibt_host(int32_t n, const int32_t *pos, const int32_t *key, const uint32_t *age, int32_t *actions,
                   uint64_t *failed) {
    if (!pos || !key || !age || !actions || !failed) return fail(MAPF_EINVAL, "null argument");
    if (n < 1 || n > 64) return fail(MAPF_EINVAL, "n must be in 1..64");
    constexpr long NONE = -(1L << 40);
    long cell[64], nxt[64];
    int cand[64][NA], ncand[64], cur[64], par[64], order[64];
    for (int i = 0; i < n; ++i) {
        cell[i] = (long)pos[2 * i] * (1L << 20) + pos[2 * i + 1];
        for (int j = 0; j < i; ++j)
            if (cell[j] == cell[i]) return fail(MAPF_EINVAL, "two agents on one cell");
        ncand[i] = 0;
        for (int a = 0; a < NA; ++a)
            if (key[i * NA + a] >= 0) cand[i][ncand[i]++] = a;
        std::stable_sort(cand[i], cand[i] + ncand[i], [&](int a, int b) { return key[i * NA + a] < key[i * NA + b]; });
        nxt[i] = NONE; cur[i] = 0; par[i] = -1; order[i] = i; actions[i] = 0;
    }
    std::stable_sort(order, order + n, [&](int a, int b) { return age[a] > age[b]; });
    auto target = [&](int i, int a) { return cell[i] + (long)dr(a) * (1L << 20) + dc(a); };
    uint64_t fl = 0;
    int iters = 0;
    bool bail = false;
    for (int k = 0; k < n && !bail; ++k) {
        int i = order[k];
        if (nxt[i] != NONE) continue;
        for (;;) {
            bool pushed = false, ok = false;
            const int pa = par[i];
            while (cur[i] < ncand[i]) {
                const int a = cand[i][cur[i]++];
                if (++iters > 6 * n) { bail = true; break; }
                const long q = target(i, a);
                bool taken = false;
                for (int j = 0; j < n; ++j) taken |= nxt[j] == q;
                if (taken) continue;                              // vertex
                if (pa >= 0 && q == cell[pa]) continue;           // swap with the agent that pushed
                nxt[i] = q; actions[i] = a;
                int child = -1;
                for (int j = 0; j < n; ++j)
                    if (cell[j] == q && nxt[j] == NONE) child = j;
                if (child >= 0) { par[child] = i; i = child; pushed = true; }
                else ok = true;
                break;
            }
            if (bail) {
                for (; i >= 0; i = par[i]) { nxt[i] = cell[i]; actions[i] = 0; }
                break;
            }
            if (pushed) continue;
            if (ok) break;
            nxt[i] = cell[i]; actions[i] = 0;                     // failed pick: stay
            fl |= 1ull << i;
            if (pa < 0) break;
            i = pa;                                               // backtrack
        }
    }
    *failed = fl;
    return MAPF_OK;
}

int32_t mapf_obs_bits_words(const mapf_config *cfg) {
    if (!cfg || cfg->num_channel < 1 || cfg->fov < 1) return 0;
    return obs_bits_words(cfg->num_channel, cfg->fov);
}

// The format on the host.  Agents go through in chunks: each chunk's floats become the contiguous
// bit-stream the kernels hold in LDS (bit k*CFF + j = float j of agent k, plus the spare word), and
// every output word is obs_bits_word of it -- the function obs_emit<.., OBS_BITS> stores with.
int mapf_obs_pack_host(const float *obs, int64_t n_agents, int32_t C, int32_t F, uint32_t *bits) {
    if (n_agents < 0 || C < 1 || F < 1 || C > 64 || F > 64) return fail(MAPF_EINVAL, "n_agents, C or F out of range");
    if (n_agents == 0) return MAPF_OK;
    if (!obs || !bits) return fail(MAPF_EINVAL, "null argument");
    const int CFF = C * F * F, WPA = obs_bits_words(C, F);
    constexpr int CHUNK = 256;
    std::vector<uint32_t> stream(((size_t)CHUNK * CFF + 31) / 32 + 1);
    for (int64_t a0 = 0; a0 < n_agents; a0 += CHUNK) {
        const int K = (int)std::min<int64_t>(CHUNK, n_agents - a0);
        std::fill(stream.begin(), stream.end(), 0u);
        const float *src = obs + (size_t)a0 * CFF;
        for (size_t q = 0; q < (size_t)K * CFF; ++q)
            if (src[q] != 0.f) stream[q >> 5] |= 1u << (q & 31);
        for (int k = 0; k < K; ++k)
            for (int w = 0; w < WPA; ++w) bits[((size_t)a0 + k) * WPA + w] = obs_bits_word(stream.data(), CFF, k, w);
    }
    return MAPF_OK;
}

int mapf_obs_unpack_host(const uint32_t *bits, int64_t n_agents, int32_t C, int32_t F, float *obs) {
    if (n_agents < 0 || C < 1 || F < 1 || C > 64 || F > 64) return fail(MAPF_EINVAL, "n_agents, C or F out of range");
    if (n_agents == 0) return MAPF_OK;
    if (!obs || !bits) return fail(MAPF_EINVAL, "null argument");
    const int CFF = C * F * F, WPA = obs_bits_words(C, F);
    for (int64_t a = 0; a < n_agents; ++a)
        for (int j = 0; j < CFF; ++j) obs[(size_t)a * CFF + j] = (float)obs_bits_get(bits + (size_t)a * WPA, j);
    return MAPF_OK;
}

int mapf_obs_band_skip(const mapf_config *cfg, int32_t unit, uint64_t byte_offset, uint8_t *skip, int32_t n) {
    if (!cfg || !skip || n < 0) return fail(MAPF_EINVAL, "null argument");
    if (unit != 0 && unit != 16 && unit != 64 && unit != 128) return fail(MAPF_EINVAL, "unit must be 0, 16, 64 or 128");
    if (byte_offset & 15) return fail(MAPF_EINVAL, "byte_offset must be a multiple of 16");
    if (cfg->num_agents < 1 || cfg->num_agents > 64 || cfg->fov < 1 || cfg->fov > 16 ||
        cfg->num_channel < 5 || cfg->num_channel > 7)
        return fail(MAPF_EINVAL, "num_agents, fov or num_channel out of range");
    DevEnv d{};
    d.N = cfg->num_agents; d.F = cfg->fov; d.C = cfg->num_channel; d.use_hp = cfg->use_hp;
    const int env_floats = d.N * d.C * d.F * d.F;
    if (env_floats & 3) return fail(MAPF_EINVAL, "an env's observation is not a whole number of float4s");
    if (unit == 0) unit = MAPF_BAND_UNIT;
    const int nq = env_floats >> 2;
    for (int q = 0; q < nq && q < n; ++q) skip[q] = obs_band_skip(d, unit, (size_t)byte_offset, q) ? 1 : 0;
    return nq;
}

int mapf_pace_gate(int32_t t, int32_t slack, int32_t live, int32_t *word, uint32_t *target) {
    if (!word || !target) return fail(MAPF_EINVAL, "null argument");
    if (t < 0 || slack < 0 || live < 1 || live > 64) return fail(MAPF_EINVAL, "t, slack or live out of range");
    int w = 0;
    uint32_t v = 0;
    if (!pace_gate(t, slack, live, w, v)) return 0;
    *word = w;
    *target = v;
    return 1;
}

int64_t mapf_observe_lds(const mapf_config *cfg, int32_t obs_envs, int32_t max_lds, int32_t *envs_out) {
    if (!cfg) return fail(MAPF_EINVAL, "null argument");
    if (int rc = check_config(*cfg)) return rc;
    if (obs_envs < 0 || obs_envs > 64) return fail(MAPF_EINVAL, "obs_envs must be in 0..64");
    if (max_lds < 0) return fail(MAPF_EINVAL, "max_lds must be >= 0");
    DevEnv d{};
    config_geometry(*cfg, d);
    int want = 0;
    // (no limit: the requested count as it is)
    const int envs = observe_envs(d, obs_envs, max_lds > 0 ? (size_t)max_lds : ~(size_t)0, want);
    if (envs_out) *envs_out = envs;
    if (envs < 1)
        return fail(MAPF_EINVAL, "one env's observe workgroup needs " + std::to_string(observe_launch_lds(d, 1)) +
                                     " bytes of LDS, over " + std::to_string(max_lds));
    return (int64_t)observe_launch_lds(d, envs);
}

// s waits for the deferred aux-stream searches: every one (all), or those due before the
// step about to be launched
// Deferral is off while s is captured (observe_with_search), so a pending event was recorded
// outside any capture: a captured stream cannot wait on it (the graph would depend on work
// outside itself) -- the caller must join it first (mapf_flush, or any call on an uncaptured
// stream) before beginning the capture.
static int join_deferred(mapf_env *e, hipStream_t s, bool all) {
    if (e->def_due[0] >= 0 || e->def_due[1] >= 0) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        HIPCHK(hipStreamIsCapturing(s, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(MAPF_ESTATE, "a search deferred before this stream capture began is still pending: "
                                     "call mapf_flush on an uncaptured stream before capturing");
    }
    for (int k = 0; k < 2; ++k) {
        if (e->def_due[k] >= 0 && (all || e->nsteps >= e->def_due[k])) {
            HIPCHK(hipStreamWaitEvent(s, e->ev_def[k], 0));
            e->def_due[k] = -1;
        }
    }
    return MAPF_OK;
}

// the searches that end every reset: first human paths + every agent's BFS map, then each
// human's next path
static int reset_searches(mapf_env *e, hipStream_t s) {
    const DevEnv &d = e->d;
    e->nsteps = 0;
    // the PIBT ages restart with the episode: no goal seen yet
    HIPCHK(hipMemsetAsync(e->pibt_since, 0xFF, (size_t)d.B * d.N * sizeof(uint32_t), s));
    launch_search(d, 0, 1, s);     // first human paths (buffer 0) + every agent's BFS map
    launch_plan(d, 1, s);          // promote them, plan each human's next path
    launch_search(d, 0, 2, s);     // ... and search it (buffer 1)
    HIPCHK(hipGetLastError());
    e->parity = 1;
    e->pending = -1;
    e->ready = true;
    return MAPF_OK;
}

int mapf_reset(mapf_env *e, const mapf_reset_spec *spec, void *stream) {
    if (!e || !spec || !spec->maps) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = join_deferred(e, s, true)) return rc;
    DevEnv &d = e->d;
    const int B = d.B, N = d.N, H = d.H, W = d.W;
    const size_t nmaps = d.shared_map ? 1 : (size_t)B;
    if (spec->mode != 0 && spec->mode != 1) return fail(MAPF_EINVAL, "reset mode must be 0 or 1");
    if (spec->mode == 1 && d.human_mode == 2) return fail(MAPF_EINVAL, "seeded reset needs human_mode 0 or 1");
    if (spec->mode == 1 && spec->seed) d.seed = spec->seed;

    // map values: 0 free / -1 obstacle (the padded bitmaps and static-action masks are built
    // from them on the device, launch_build_maps)
    for (size_t k = 0; k < nmaps * (size_t)H * W; ++k)
        if (spec->maps[k] != 0 && spec->maps[k] != -1) return fail(MAPF_EINVAL, "map values must be 0 (free) or -1 (obstacle)");
    auto free_at = [&](int b, int r, int c) {
        if (r < 0 || r >= H || c < 0 || c >= W) return false;
        const size_t m = d.shared_map ? 0 : (size_t)b;
        return spec->maps[m * H * W + r * W + c] == 0;
    };

    std::vector<uint32_t> seq, hpos, hgoal, hseq;
    std::vector<int32_t> seq_len, hseq_len;
    if (spec->mode == 0) {
        if (!spec->seq || !spec->seq_len) return fail(MAPF_EINVAL, "mode 0 needs seq and seq_len");
        seq.assign((size_t)B * N * d.S, 0u);
        seq_len.assign((size_t)B * N, 0);
        for (int b = 0; b < B; ++b) {
            std::vector<uint32_t> starts;
            for (int i = 0; i < N; ++i) {
                const size_t ai = (size_t)b * N + i;
                const int len = spec->seq_len[ai];
                if (len < 1 || len > d.S) return fail(MAPF_EINVAL, "seq_len out of range");
                seq_len[ai] = len;
                for (int k = 0; k < len; ++k) {
                    const int r = spec->seq[(ai * d.S + k) * 2], c = spec->seq[(ai * d.S + k) * 2 + 1];
                    if (r < 0 || r >= H || c < 0 || c >= W) return fail(MAPF_EINVAL, "sequence cell out of the map");
                    seq[ai * d.S + k] = pack(r, c);
                }
                const int r0 = spec->seq[(ai * d.S) * 2], c0 = spec->seq[(ai * d.S) * 2 + 1];
                if (!free_at(b, r0, c0)) return fail(MAPF_EINVAL, "agent start on an obstacle");
                for (uint32_t s2 : starts)
                    if (s2 == pack(r0, c0)) return fail(MAPF_EINVAL, "two agents start on the same cell");
                starts.push_back(pack(r0, c0));
            }
        }
        hpos.assign(B, 0u); hgoal.assign(B, 0u);
        if (d.human_mode == 2) {
            if (!spec->human_seq || !spec->human_seq_len) return fail(MAPF_EINVAL, "human_mode 2 needs human_seq");
            hseq.assign((size_t)B * d.HS, 0u);
            hseq_len.assign(B, 0);
            for (int b = 0; b < B; ++b) {
                const int len = spec->human_seq_len[b];
                if (len < 2 || len > d.HS) return fail(MAPF_EINVAL, "human_seq_len out of range");
                hseq_len[b] = len;
                for (int k = 0; k < len; ++k) {
                    const int r = spec->human_seq[((size_t)b * d.HS + k) * 2], c = spec->human_seq[((size_t)b * d.HS + k) * 2 + 1];
                    if (!free_at(b, r, c)) return fail(MAPF_EINVAL, "human pose not on a free cell");
                    hseq[(size_t)b * d.HS + k] = pack(r, c);
                }
            }
        } else {
            if (!spec->human_start || !spec->human_goal) return fail(MAPF_EINVAL, "mode 0 needs human_start/goal");
            for (int b = 0; b < B; ++b) {
                const int sr = spec->human_start[2 * b], sc = spec->human_start[2 * b + 1];
                const int gr = spec->human_goal[2 * b], gc = spec->human_goal[2 * b + 1];
                if (!free_at(b, sr, sc) || !free_at(b, gr, gc)) return fail(MAPF_EINVAL, "human start/goal not free");
                if (sr == gr && sc == gc) return fail(MAPF_EINVAL, "human start == goal (astar_4 returns [])");
                hpos[b] = pack(sr, sc);
                hgoal[b] = pack(gr, gc);
            }
        }
    }

    HIPCHK(hipMemcpyAsync(e->maps8, spec->maps, nmaps * (size_t)H * W, hipMemcpyHostToDevice, s));
    launch_build_maps(d, e->maps8, s);
    HIPCHK(hipMemsetAsync(d.counters, 0, C_NUM * sizeof(uint32_t), s));
    if (spec->mode == 0) {
        HIPCHK(hipMemcpyAsync(d.seq, seq.data(), seq.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.seq_len, seq_len.data(), seq_len.size() * 4, hipMemcpyHostToDevice, s));
        if (d.human_mode == 2) {
            HIPCHK(hipMemcpyAsync(d.hseq, hseq.data(), hseq.size() * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d.hseq_len, hseq_len.data(), hseq_len.size() * 4, hipMemcpyHostToDevice, s));
        } else {
            HIPCHK(hipMemcpyAsync(d.hpos, hpos.data(), hpos.size() * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d.hgoal, hgoal.data(), hgoal.size() * 4, hipMemcpyHostToDevice, s));
        }
        launch_reset_fixed(d, s);
    } else {
        launch_reset_seeded(d, s);
    }
    const int rc = reset_searches(e, s);
    if (rc != MAPF_OK) return rc;
    HIPCHK(hipStreamSynchronize(s));   // host staging buffers die at return
    return MAPF_OK;
}

int mapf_reset_generated(mapf_env *e, const mapf_mapgen_spec *spec, int8_t *maps_out, void *stream) {
    if (!e || !spec) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = join_deferred(e, s, true)) return rc;
    DevEnv &d = e->d;
    if (d.human_mode == 2) return fail(MAPF_EINVAL, "generated maps need human_mode 0 or 1 (seeded reset)");
    MapGen g{spec->kind, spec->lo, spec->hi, spec->largest ? 1 : 0, spec->density, spec->epoch,
             spec->seed ? spec->seed : d.seed};
    if (spec->kind == MAPF_MAPS_WAREHOUSE) {
        if (spec->lo < 3 || spec->hi < spec->lo) return fail(MAPF_EINVAL, "warehouse length range [lo, hi] invalid");
        const int breadth = (int)((double)spec->hi / (2.0 / 3.0));
        if (d.H < spec->hi || d.W < breadth) return fail(MAPF_EINVAL, "the H x W stack is smaller than the longest warehouse");
    } else if (spec->kind == MAPF_MAPS_RANDOM) {
        if (!(spec->density >= 0.f && spec->density <= 1.f)) return fail(MAPF_EINVAL, "density must be in [0, 1]");
    } else {
        return fail(MAPF_EINVAL, "unknown map kind");
    }
    if (spec->largest && d.H * d.W > LC_MAX_CELLS) return fail(MAPF_EINVAL, "largest component: at most 8192 cells");
    if (spec->seed) d.seed = spec->seed;
    const size_t nmaps = d.shared_map ? 1 : (size_t)d.B;
    launch_mapgen(d, g, e->maps8, s);
    if (maps_out)
        HIPCHK(hipMemcpyAsync(maps_out, e->maps8, nmaps * (size_t)d.H * d.W, hipMemcpyDeviceToDevice, s));
    launch_build_maps(d, e->maps8, s);
    HIPCHK(hipMemsetAsync(d.counters, 0, C_NUM * sizeof(uint32_t), s));
    launch_reset_seeded(d, s);
    return reset_searches(e, s);       // asynchronous: nothing on the host to keep alive
}

// the device pointers of a mapf_step_out (NULL: none)
static StepOut step_out_of(const mapf_step_out *out) {
    StepOut o{};
    if (out) {
        o.status = out->status; o.reward = out->reward; o.shadow_goals = out->shadow_goals; o.cost = out->cost;
        o.train_valid = out->train_valid; o.actions_fixed = out->actions_fixed; o.goals_reached = out->goals_reached;
        o.constraints = out->constraints; o.reward_total = out->reward_total;
    }
    return o;
}

static int step_impl(mapf_env *e, int32_t *actions, const mapf_step_out *out, uint32_t flags, void *stream) {
    if (!e || !actions) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_step before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const StepOut o = step_out_of(out);
    if (e->pending >= 0) {             // previous step's search work was not observed-through
        if (int rc = join_deferred(e, s, true)) return rc;
        launch_search(e->d, e->pending, 0, s);
        e->pending = -1;
    }
    if (int rc = join_deferred(e, s, !(flags & MAPF_STEP_COMMIT))) return rc;
    const int parity = e->parity;
    launch_step(e->d, actions, o, flags, parity, s);
    if (flags & MAPF_STEP_COMMIT) {
        if (e->d.human_mode != 0 || e->d.keep_bfs) e->pending = parity;
        e->parity = (parity + 1) % 3;
        ++e->nsteps;
    }
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

static int flush_search(mapf_env *e, hipStream_t s) {
    if (int rc = join_deferred(e, s, true)) return rc;
    if (e->pending >= 0) {
        launch_search(e->d, e->pending, 0, s);
        e->pending = -1;
        HIPCHK(hipGetLastError());
    }
    return MAPF_OK;
}

int mapf_step(mapf_env *e, const int32_t *actions, const mapf_step_out *out, uint32_t flags, void *stream) {
    return step_impl(e, const_cast<int32_t *>(actions), out, flags & MAPF_STEP_COMMIT, stream);
}

int mapf_step_random(mapf_env *e, int32_t *actions_out, const mapf_step_out *out, uint32_t flags, void *stream) {
    return step_impl(e, actions_out, out, (flags & MAPF_STEP_COMMIT) | 2u, stream);
}

// The pending search (the last step's BFS maps and human paths) beside the observe launch,
// forked off s onto two streams.  Nothing the observation reads is written by the search
// except the listed agents' BFS maps (C = 7): those are searched on e->aux, joined right
// after the observe launch, and exactly their BFS channel is then rewritten (bfs_fixup).
// The rest -- the humans' next paths, and BFS maps without the BFS channel -- runs on
// e->aux2 and stays there past this call (join_deferred), unless s is being captured into
// a graph (a capture must join every fork before it ends).
static int observe_with_search(mapf_env *e, float *obs, float *vec, hipStream_t s) {
    if (!e->aux) {
        HIPCHK(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&e->aux2, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_join2, hipEventDisableTiming));
        for (hipEvent_t &ev : e->ev_def) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    const bool defer = !e->tune.no_defer && cap == hipStreamCaptureStatusNone;
    const bool bfsch = e->d.C >= 7 && e->d.keep_bfs;
    const int parity = e->pending;
    e->pending = -1;
    HIPCHK(hipEventRecord(e->ev_fork, s));
    if (bfsch) {
        HIPCHK(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        launch_search(e->d, parity, 4, e->aux);                 // the BFS maps the observation reads
        HIPCHK(hipEventRecord(e->ev_join, e->aux));
    }
    HIPCHK(hipStreamWaitEvent(e->aux2, e->ev_fork, 0));
    launch_search(e->d, parity, bfsch ? 3 : 0, e->aux2);        // human paths (+ BFS maps without the channel)
    if (defer) {
        // slot k's previous search was due before an earlier step: joined by now
        const int k = e->def_next;
        HIPCHK(hipEventRecord(e->ev_def[k], e->aux2));
        e->def_due[k] = e->nsteps + 1;
        e->def_next = k ^ 1;
    } else {
        HIPCHK(hipEventRecord(e->ev_join2, e->aux2));
    }
    launch_observe(e->d, obs, vec, 0, parity, s);
    if (bfsch) {
        HIPCHK(hipStreamWaitEvent(s, e->ev_join, 0));
        launch_bfs_fixup(e->d, parity, obs, s);
    }
    if (!defer) HIPCHK(hipStreamWaitEvent(s, e->ev_join2, 0));
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// bits: obs is the packed uint32 [B][N][WPA] buffer (mapf_observe_bits)
static int observe_impl(mapf_env *e, float *obs, float *vec, void *stream, bool bits) {
    if (!e || !obs || !vec) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_observe before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int nsearch = 0, parity = 0;
    if (e->pending >= 0) {
        if (!observe_hosts_search(e->d) || e->d.C >= 7) {   // wide grids / BFS channel: search beside the launch
            // the forked form ends in launch_bfs_fixup, which rewrites channel 6 as FLOATS (32 times a
            // packed buffer's size): a packed call always joins the search first (mapf.h)
            if (!e->tune.serial_search && !bits) return observe_with_search(e, obs, vec, s);
            if (int rc = flush_search(e, s)) return rc;
        } else {                       // search work rides in the observe launch
            nsearch = e->d.search_blocks;
            parity = e->pending;
            e->pending = -1;
        }
    }
    launch_observe(e->d, obs, vec, nsearch, parity, s, bits);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_observe(mapf_env *e, float *obs, float *vec, void *stream) { return observe_impl(e, obs, vec, stream, false); }
int mapf_observe_bits(mapf_env *e, uint32_t *bits, float *vec, void *stream) {
    return observe_impl(e, reinterpret_cast<float *>(bits), vec, stream, true);
}

static int step_observe_impl(mapf_env *e, int32_t *actions, const mapf_step_out *out, uint32_t flags, float *obs,
                             float *vec, void *stream, bool bits = false) {
    if (!e || !actions || !obs || !vec) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_step_observe before mapf_reset");
    if (!step_observe_fusable(e->d)) {          // two launches, same results
        if (int rc = step_impl(e, actions, out, MAPF_STEP_COMMIT | flags, stream)) return rc;
        return observe_impl(e, obs, vec, stream, bits);
    }
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = join_deferred(e, s, true)) return rc;
    ++e->nsteps;
    const StepOut o = step_out_of(out);
    const bool host = observe_hosts_search(e->d);
    int nsearch = 0, sslot = 0;
    if (e->pending >= 0) {
        if (host) { nsearch = e->d.search_blocks; sslot = e->pending; }
        else launch_search(e->d, e->pending, 0, s);
        e->pending = -1;
    }
    const int parity = e->parity;
    launch_step_observe(e->d, actions, o, MAPF_STEP_COMMIT | flags, parity, obs, vec, nsearch, sslot, s, bits);
    if (e->d.human_mode != 0 || e->d.keep_bfs) {
        if (host) e->pending = parity;             // rides in the next launch
        else launch_search(e->d, parity, 0, s);
    }
    e->parity = (parity + 1) % 3;
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_step_observe(mapf_env *e, const int32_t *actions, const mapf_step_out *out, float *obs, float *vec,
                      void *stream) {
    return step_observe_impl(e, const_cast<int32_t *>(actions), out, 0u, obs, vec, stream);
}

int mapf_step_observe_bits(mapf_env *e, const int32_t *actions, const mapf_step_out *out, uint32_t *bits, float *vec,
                           void *stream) {
    return step_observe_impl(e, const_cast<int32_t *>(actions), out, 0u, reinterpret_cast<float *>(bits), vec, stream, true);
}

int mapf_step_observe_random(mapf_env *e, int32_t *actions_out, const mapf_step_out *out, float *obs, float *vec,
                             void *stream) {
    return step_observe_impl(e, actions_out, out, 2u, obs, vec, stream);
}

// slot k of rollout output buffers (NULL members stay NULL)
static mapf_step_out step_out_slot(const mapf_step_out &out, size_t k, const DevEnv &d) {
    const size_t BN = (size_t)d.B * d.N;
    auto adv = [&](auto *p, size_t n) { return p ? p + k * n : p; };
    mapf_step_out ot{};
    ot.status = adv(out.status, BN); ot.reward = adv(out.reward, BN);
    ot.shadow_goals = adv(out.shadow_goals, (size_t)d.B); ot.cost = adv(out.cost, BN);
    ot.train_valid = adv(out.train_valid, BN * 5); ot.actions_fixed = adv(out.actions_fixed, BN);
    ot.goals_reached = adv(out.goals_reached, BN); ot.constraints = adv(out.constraints, BN);
    ot.reward_total = adv(out.reward_total, BN);
    return ot;
}

// what every call that runs a policy checks after its own arguments (`name`, for the error text)
static int policy_ready(const mapf_env *e, int policy, const char *name) {
    if (needs_bfs(policy) && !e->d.keep_bfs) return fail(MAPF_ESTATE, "keep_bfs is off");
    if (!e->ready) return fail(MAPF_ESTATE, std::string(name) + " before mapf_reset");
    return MAPF_OK;
}

// the policy's pick into act [B][N]: descent's or PIBT's launch; nothing for the random policy (the step
// draws) and the tape
static int policy_pick(mapf_env *e, int policy, int32_t *act, hipStream_t s) {
    if (!needs_bfs(policy)) return MAPF_OK;
    if (int rc = flush_search(e, s)) return rc;      // the maps of the last step's new goals
    if (policy == ROLLOUT_DESCENT) launch_descent_actions(e->d, act, s);
    else launch_pibt_actions(e->d, act, e->pibt_seen, e->pibt_since, s);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

static int policy_actions(mapf_env *e, int policy, const char *name, int32_t *actions, void *stream) {
    if (!e || !actions) return fail(MAPF_EINVAL, "null argument");
    if (int rc = policy_ready(e, policy, name)) return rc;
    HIPCHK(hipSetDevice(e->device));
    return policy_pick(e, policy, actions, (hipStream_t)stream);
}
int mapf_descent_actions(mapf_env *e, int32_t *actions, void *stream) {
    return policy_actions(e, ROLLOUT_DESCENT, "mapf_descent_actions", actions, stream);
}
int mapf_pibt_actions(mapf_env *e, int32_t *actions, void *stream) {
    return policy_actions(e, ROLLOUT_PIBT, "mapf_pibt_actions", actions, stream);
}

int mapf_pibt_human_cells(mapf_env *e, uint32_t *cells, void *stream) {
    if (!e || !cells) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_pibt_human_cells before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    // the current path only: the path that follows may still be searched beside the step (join_deferred)
    launch_pibt_human_cells(e->d, cells, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// ROUTE_STEPS: T x (the policy's pick, with action noise mapf_noise_actions' launch into the handle's row, a
// committed step), same results as the one-launch kernels.  An
// observing request's step is step_observe into slot t (or in place; the tape plays row t whatever `slots`
// says).  A perf request's is a step into the handle's step scratch and the record's accumulate over it.
// out: the caller's outputs as q.out holds them.
static int rollout_steps(mapf_env *e, const RolloutReq &q, const mapf_step_out *out, void *stream) {
    const bool perf = q.form == ROLLOUT_PERF, bits = (q.slots & MAPF_SLOTS_OBS_BITS) != 0;
    // with MAPF_SLOTS_OBS_BITS `obs` is the packed buffer (uint32 behind the float pointer): a slot is
    // B * N * WPA words, and step_observe is told so
    const size_t BN = (size_t)e->d.B * e->d.N;
    const size_t obs_t = bits ? BN * (size_t)obs_bits_words(e->d.C, e->d.F) : BN * e->d.C * e->d.F * e->d.F;
    if (perf && !e->perf_step.status) return fail(MAPF_ESTATE, "no step scratch on this handle");
    const uint32_t draw = q.policy == ROLLOUT_RANDOM ? 2u : 0u;
    for (int32_t t = 0; t < q.T; ++t) {
        const size_t k = (q.slots & 1) ? (size_t)t : 0;
        int32_t *act = q.actions ? q.actions + (q.policy == ROLLOUT_TAPE ? (size_t)t : k) * BN : e->perf_act;
        if (int rc = policy_pick(e, q.policy, act, (hipStream_t)stream)) return rc;
        if (needs_bfs(q.policy) && e->d.noise_q16 != 0) {      // the label stays in the row picked into; the step plays the scratch row
            launch_noise_actions(e->d, act, e->noise_act, (hipStream_t)stream);
            act = e->noise_act;
        }
        if (perf) {
            if (int rc = step_impl(e, act, &e->perf_step, MAPF_STEP_COMMIT | draw, stream)) return rc;
            launch_perf_accumulate(step_out_of(&e->perf_step), 1, e->d.B, e->d.N, q.perf, t == 0 ? q.accumulate : 1,
                                   (hipStream_t)stream);
        } else {
            mapf_step_out ot{};
            if (out) ot = step_out_slot(*out, k, e->d);
            if (int rc = step_observe_impl(e, act, out ? &ot : nullptr, draw, q.obs + k * obs_t, q.vec + k * BN * 4, stream, bits))
                return rc;
        }
    }
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// A checked request on its route (rollout_plan's switch): one launch, or rollout_steps
static int rollout_run(mapf_env *e, RolloutReq &q, const mapf_step_out *out, void *stream) {
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (q.T == 0) return MAPF_OK;
    q.pibt_seen = e->pibt_seen;
    q.pibt_since = e->pibt_since;
    const bool perf = q.form == ROLLOUT_PERF;
    const int route = rollout_route(e->d, q);
    if (route == ROUTE_STEPS) return rollout_steps(e, q, out, stream);
    if (int rc = flush_search(e, s)) return rc;     // the kernel searches inline from here on
    const int rc = route == ROUTE_PAIRS ? (perf ? launch_rollout_perf : launch_rollout_random)(e->d, q, e->tune, e->args, s)
                                        : (perf ? launch_rollout_wide_perf : launch_rollout_wide)(e->d, q, e->tune, e->args, s);
    if (rc == MAPF_ESTATE)
        return fail(MAPF_ESTATE, "every argument slot for captured persistent launches of this handle is taken "
                                 "(16 per handle, ArgRing; mapf_release_captures frees them)");
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// mapf_rollout_random / _actions / _descent / _pibt / _sparse (`name`, for the error text).  policy (ROLLOUT_*)
// says where the actions come from; `actions` is the caller's tape with ROLLOUT_TAPE (read only), else out.
// shadow / valid: mapf_rollout_sparse's (NULL: every other entry point)
static int rollout_impl(mapf_env *e, int policy, const char *name, int32_t T, int32_t slots, int32_t *actions,
                        const mapf_step_out *out, float *obs, float *vec, void *stream, uint32_t *shadow = nullptr,
                        int32_t valid = 0) {
    if (!e || !actions || !obs || !vec) return fail(MAPF_EINVAL, "null argument");
    if (T < 0) return fail(MAPF_EINVAL, "T must be >= 0");
    if (slots < 0 || slots > (MAPF_SLOTS | MAPF_SLOTS_BAND_CLEAN | MAPF_SLOTS_OBS_BITS)) return fail(MAPF_EINVAL, "slots: unknown bits");
    if (int rc = policy_ready(e, policy, name)) return rc;
    if (policy == ROLLOUT_TAPE && out && out->actions_fixed && T > 0) {      // the tape is read while actions_fixed is written
        const size_t BN = (size_t)e->d.B * e->d.N;
        const uintptr_t a0 = (uintptr_t)actions, a1 = a0 + (size_t)T * BN * 4;
        const uintptr_t f0 = (uintptr_t)out->actions_fixed, f1 = f0 + ((slots & 1) ? (size_t)T : 1) * BN * 4;
        if (a0 < f1 && f0 < a1) return fail(MAPF_EINVAL, "actions_in overlaps out->actions_fixed");
    }
    RolloutReq q{};
    q.form = shadow ? ROLLOUT_SPARSE : ROLLOUT_OBSERVE;
    q.policy = policy;
    q.T = T;
    q.slots = slots;
    q.actions = actions;
    q.out = step_out_of(out);
    q.obs = obs;
    q.vec = vec;
    q.shadow = shadow;
    q.valid = valid;
    return rollout_run(e, q, out, stream);
}

int mapf_rollout_random(mapf_env *e, int32_t T, int32_t slots, int32_t *actions_out, const mapf_step_out *out,
                        float *obs, float *vec, void *stream) {
    return rollout_impl(e, ROLLOUT_RANDOM, "mapf_rollout_random", T, slots, actions_out, out, obs, vec, stream);
}

int mapf_rollout_actions(mapf_env *e, int32_t T, int32_t slots, const int32_t *actions_in, const mapf_step_out *out,
                         float *obs, float *vec, void *stream) {
    // the TAPE kernels only read it
    return rollout_impl(e, ROLLOUT_TAPE, "mapf_rollout_actions", T, slots, const_cast<int32_t *>(actions_in), out, obs,
                        vec, stream);
}

int mapf_rollout_descent(mapf_env *e, int32_t T, int32_t slots, int32_t *actions_out, const mapf_step_out *out,
                         float *obs, float *vec, void *stream) {
    return rollout_impl(e, ROLLOUT_DESCENT, "mapf_rollout_descent", T, slots, actions_out, out, obs, vec, stream);
}

int mapf_rollout_pibt(mapf_env *e, int32_t T, int32_t slots, int32_t *actions_out, const mapf_step_out *out,
                      float *obs, float *vec, void *stream) {
    return rollout_impl(e, ROLLOUT_PIBT, "mapf_rollout_pibt", T, slots, actions_out, out, obs, vec, stream);
}

int mapf_rollout_sparse(mapf_env *e, int32_t policy, int32_t T, int32_t *actions, const mapf_step_out *out, float *obs,
                        float *vec, uint32_t *shadow, int32_t valid, void *stream) {
    if (int rc = check_policy(policy)) return rc;
    if (!shadow) return fail(MAPF_EINVAL, "null argument");
    if (valid < 0) return fail(MAPF_EINVAL, "valid must be >= 0");
    if ((uintptr_t)shadow & 63) return fail(MAPF_EINVAL, "shadow must be 64-byte aligned");
    // where the sparse form does not take the launch it is the band-clean one: the band's pieces are
    // zeros over zeros in every slot the shadow describes, but only there
    const int32_t slots = MAPF_SLOTS | (valid >= T ? MAPF_SLOTS_BAND_CLEAN : 0);
    return rollout_impl(e, policy, "mapf_rollout_sparse", T, slots, actions, out, obs, vec, stream, shadow, valid);
}

int mapf_rollout_perf(mapf_env *e, int32_t policy, int32_t T, int32_t *actions, mapf_perf *perf, int32_t accumulate,
                      void *stream) {
    if (!e || !perf) return fail(MAPF_EINVAL, "null argument");
    if (int rc = check_policy(policy)) return rc;
    if (policy == ROLLOUT_TAPE && !actions) return fail(MAPF_EINVAL, "the tape policy needs actions");
    if (T < 0) return fail(MAPF_EINVAL, "T must be >= 0");
    if (int rc = policy_ready(e, policy, "mapf_rollout_perf")) return rc;
    RolloutReq q{};
    q.form = ROLLOUT_PERF;
    q.policy = policy;
    q.T = T;
    q.slots = actions ? 1 : 0;      // the kernels' picks go to the caller's [T][B][N]; with none they are stored nowhere
    q.actions = actions;
    q.perf = perf;
    q.accumulate = accumulate != 0;
    return rollout_run(e, q, nullptr, stream);
}

int mapf_obs_sparse_applies(const mapf_config *cfg, uint64_t obs_address) {
    if (!cfg) return fail(MAPF_EINVAL, "null argument");
    if (cfg->num_agents < 1 || cfg->num_agents > 64 || cfg->fov < 1 || cfg->fov > 16 || cfg->num_channel < 5 ||
        cfg->num_channel > 7)
        return fail(MAPF_EINVAL, "num_agents, fov or num_channel out of range");
    return obs_sparse_applies(cfg->num_agents, cfg->num_channel, cfg->fov, (size_t)obs_address) ? 1 : 0;
}

int mapf_release_captures(mapf_env *e) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    e->args.release_captures();
    return MAPF_OK;
}

int mapf_flush(mapf_env *e, void *stream) {
    if (!e) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    return flush_search(e, (hipStream_t)stream);
}

int mapf_random_actions(mapf_env *e, int32_t *actions, void *stream) {
    if (!e || !actions) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_random_actions before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    launch_random_actions(e->d, actions, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_noise_actions(mapf_env *e, const int32_t *labels, int32_t *played, void *stream) {
    if (!e || !labels || !played) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_noise_actions before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    launch_noise_actions(e->d, labels, played, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_bfs(mapf_env *e, int16_t *dist, void *stream) {
    if (!e || !dist) return fail(MAPF_EINVAL, "null argument");
    if (!e->d.keep_bfs) return fail(MAPF_ESTATE, "keep_bfs is off");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = flush_search(e, (hipStream_t)stream)) return rc;
    launch_bfs_export(e->d, dist, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// hsv_to_rgb(h, 1, 1) (matplotlib.colors, util.init_colors) * 255, truncated like astype('uint8')
static void hue_rgb(double h, uint8_t *rgb) {
    const double h6 = h * 6.0;
    const int i = (int)std::floor(h6) % 6;
    const double f = h6 - std::floor(h6), q = 1.0 - f, t = f;
    double r, g, b;
    switch (i) {
        case 0: r = 1; g = t; b = 0; break;
        case 1: r = q; g = 1; b = 0; break;
        case 2: r = 0; g = 1; b = t; break;
        case 3: r = 0; g = q; b = 1; break;
        case 4: r = t; g = 0; b = 1; break;
        default: r = 1; g = 0; b = q; break;
    }
    rgb[0] = (uint8_t)(r * 255.0); rgb[1] = (uint8_t)(g * 255.0); rgb[2] = (uint8_t)(b * 255.0);
}

int mapf_render(mapf_env *e, const int32_t *envs, int32_t n, int32_t scale, uint8_t *frames, void *stream) {
    if (!e || !envs || !frames) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_render before mapf_reset");
    if (n < 0 || n > 65535) return fail(MAPF_EINVAL, "n must be in 0..65535");
    if (scale < 4 || scale > 64) return fail(MAPF_EINVAL, "scale must be in 4..64");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = flush_search(e, s)) return rc;
    if (n == 0) return MAPF_OK;
    RenderSpec rs{};
    rs.scale = scale;
    const uint8_t fixed[9] = {255, 255, 255, 0, 0, 0, 127, 127, 127};   // colours[0], [-1], [-2] * 255
    std::memcpy(rs.palette, fixed, 9);
    for (int a = 0; a < e->d.N; ++a) hue_rgb((double)a / (double)e->d.N, rs.palette + 3 * (3 + a));
    // drawStar(coord, S, S, 5): outerRad = S // 2, innerRad = int(outerRad * 3 / 8)
    const double PI = 3.141592653589793, between = 2.0 * PI / 5.0;
    const int outer = scale / 2, inner = (int)(outer * 3.0 / 8.0);
    for (int i = 0; i < 5; ++i) {
        const double pa = PI / 2.0 + i * between;
        const double ang[3] = {pa - between / 2.0, pa, pa + between / 2.0};
        const int rad[3] = {inner, outer, inner};
        for (int k = 0; k < 3; ++k) {
            rs.star_x[3 * i + k] = rad[k] * std::cos(ang[k]);
            rs.star_y[3 * i + k] = rad[k] * std::sin(ang[k]);
        }
    }
    launch_render(e->d, envs, n, rs, frames, s);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_get_counters(mapf_env *e, uint32_t *host16, void *stream) {
    if (!e || !host16) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = flush_search(e, s)) return rc;
    HIPCHK(hipMemcpyAsync(host16, e->d.counters, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAPF_OK;
}

int mapf_get_profile(mapf_env *e, uint64_t *host16, int reset, void *stream) {
    if (!e || !host16) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<uint64_t> all(PROF_TL);
    HIPCHK(hipMemcpyAsync(all.data(), e->d.prof, all.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(e->d.prof, 0, PROF_WORDS * sizeof(uint64_t), s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 16; ++k) host16[k] = 0;
    for (size_t w = 0; w < 65536; ++w) {   // sums over waves of the LAST launch; [15] = waves
        if (!all[w * 8 + 7]) continue;
        for (int k = 0; k < 7; ++k) host16[k] += all[w * 8 + k];
        host16[15] += 1;
    }
    return MAPF_OK;
}

int mapf_get_wave_profile(mapf_env *e, uint64_t *host, int32_t nwaves, void *stream) {
    if (!e || !host || nwaves < 0 || nwaves > (int)PROF_WAVES) return fail(MAPF_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host, e->d.prof, (size_t)nwaves * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAPF_OK;
}

int mapf_get_timeline(mapf_env *e, uint64_t *host, int32_t nblocks, void *stream) {
    if (!e || !host || nblocks < 0 || nblocks > (int)PROF_TL_BLOCKS) return fail(MAPF_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host, e->d.prof + PROF_TL, (size_t)nblocks * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MAPF_OK;
}

int mapf_get_state(mapf_env *e, const mapf_state *h, void *stream) {
    if (!e || !h) return fail(MAPF_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const DevEnv &d = e->d;
    const size_t BN = (size_t)d.B * d.N;
    std::vector<uint32_t> pos(BN), goal(BN), hpath((size_t)d.B * 2 * d.Lmax), hp(d.B), hn(d.B), hg(d.B), he(d.B), clk(d.B);
    std::vector<int8_t> la(BN);
    std::vector<int32_t> cur(BN), hl(2 * (size_t)d.B), hs(d.B), hc(d.B);
    if (int rc = flush_search(e, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(pos.data(), d.pos, BN * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(goal.data(), d.goal, BN * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(la.data(), d.last_act, BN, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cur.data(), d.seq_cur, BN * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hpath.data(), d.hpath, hpath.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hl.data(), d.hlen, 2 * d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hs.data(), d.hstep, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hc.data(), d.hcur, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hn.data(), d.hnext, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hp.data(), d.hpos, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hg.data(), d.hgoal, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(he.data(), d.hentr, d.B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(clk.data(), d.clock, d.B * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < BN; ++k) {
        if (h->pos) { h->pos[2 * k] = prow(pos[k]); h->pos[2 * k + 1] = pcol(pos[k]); }
        if (h->goal) { h->goal[2 * k] = prow(goal[k]); h->goal[2 * k + 1] = pcol(goal[k]); }
        if (h->last_action) h->last_action[k] = la[k];
        if (h->seq_cursor) h->seq_cursor[k] = cur[k];
    }
    for (int b = 0; b < d.B; ++b) {
        const uint32_t *path = hpath.data() + ((size_t)b * 2 + hc[b]) * d.Lmax;
        const int st = hs[b], len = hl[2 * b + hc[b]];
        const uint32_t nx = hn[b];
        if (h->human) {
            int32_t *o = h->human + 10 * b;
            o[0] = prow(hp[b]); o[1] = pcol(hp[b]); o[2] = prow(nx); o[3] = pcol(nx);
            o[4] = prow(hg[b]); o[5] = pcol(hg[b]); o[6] = st; o[7] = len; o[8] = prow(he[b]); o[9] = pcol(he[b]);
        }
        if (h->human_path)
            for (int k = 0; k < d.Lmax; ++k) {
                h->human_path[((size_t)b * d.Lmax + k) * 2] = k < len ? prow(path[k]) : -1;
                h->human_path[((size_t)b * d.Lmax + k) * 2 + 1] = k < len ? pcol(path[k]) : -1;
            }
        if (h->clock) h->clock[b] = clk[b];
    }
    return MAPF_OK;
}

int mapf_set_state(mapf_env *e, const mapf_state *h, void *stream) {
    if (!e || !h) return fail(MAPF_EINVAL, "null argument");
    if (!e->ready) return fail(MAPF_ESTATE, "mapf_set_state before mapf_reset");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    DevEnv &d = e->d;
    const size_t BN = (size_t)d.B * d.N;
    if (int rc = flush_search(e, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    // a restored state is another point of another episode: the PIBT ages restart (mapf.h)
    HIPCHK(hipMemsetAsync(e->pibt_since, 0xFF, BN * sizeof(uint32_t), s));
    if (h->pos) {
        std::vector<uint32_t> v(BN);
        for (size_t k = 0; k < BN; ++k) {
            const int r = h->pos[2 * k], c = h->pos[2 * k + 1];
            if (r < 0 || r >= d.H || c < 0 || c >= d.W) return fail(MAPF_EINVAL, "pos out of the map");
            v[k] = pack(r, c);
        }
        HIPCHK(hipMemcpy(d.pos, v.data(), BN * 4, hipMemcpyHostToDevice));
    }
    if (h->goal) {
        std::vector<uint32_t> v(BN);
        for (size_t k = 0; k < BN; ++k) {
            const int r = h->goal[2 * k], c = h->goal[2 * k + 1];
            if (r < 0 || r >= d.H || c < 0 || c >= d.W) return fail(MAPF_EINVAL, "goal out of the map");
            v[k] = pack(r, c);
        }
        HIPCHK(hipMemcpy(d.goal, v.data(), BN * 4, hipMemcpyHostToDevice));
    }
    if (h->last_action) {
        std::vector<int8_t> v(BN);
        for (size_t k = 0; k < BN; ++k) {
            if (h->last_action[k] < -1 || h->last_action[k] > 4) return fail(MAPF_EINVAL, "last_action out of range");
            v[k] = (int8_t)h->last_action[k];
        }
        HIPCHK(hipMemcpy(d.last_act, v.data(), BN, hipMemcpyHostToDevice));
    }
    if (h->seq_cursor) HIPCHK(hipMemcpy(d.seq_cur, h->seq_cursor, BN * 4, hipMemcpyHostToDevice));
    if (h->human_path && h->human) {
        // the given path becomes buffer 0 (current); buffer 1 is re-planned below
        std::vector<uint32_t> path((size_t)d.B * 2 * d.Lmax, 0u);
        std::vector<int32_t> hl(2 * (size_t)d.B, 1), hc(d.B, 0);
        for (int b = 0; b < d.B; ++b) {
            const int len = h->human[10 * b + 7];
            if (len < 1 || len > d.Lmax) return fail(MAPF_EINVAL, "human path length out of range");
            hl[2 * b] = len;
            for (int k = 0; k < len; ++k)
                path[(size_t)b * 2 * d.Lmax + k] = pack(h->human_path[((size_t)b * d.Lmax + k) * 2],
                                                        h->human_path[((size_t)b * d.Lmax + k) * 2 + 1]);
        }
        HIPCHK(hipMemcpy(d.hpath, path.data(), path.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.hlen, hl.data(), hl.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.hcur, hc.data(), d.B * 4, hipMemcpyHostToDevice));
    }
    if (h->human) {
        std::vector<uint32_t> hp(d.B), hg(d.B), he(d.B);
        std::vector<int32_t> hs(d.B);
        for (int b = 0; b < d.B; ++b) {
            const int32_t *o = h->human + 10 * b;
            hp[b] = pack(o[0], o[1]); hg[b] = pack(o[4], o[5]); hs[b] = o[6]; he[b] = pack(o[8], o[9]);
        }
        HIPCHK(hipMemcpy(d.hpos, hp.data(), d.B * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.hgoal, hg.data(), d.B * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.hstep, hs.data(), d.B * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.hentr, he.data(), d.B * 4, hipMemcpyHostToDevice));
    }
    if (h->clock) HIPCHK(hipMemcpy(d.clock, h->clock, d.B * 4, hipMemcpyHostToDevice));
    if (h->human || h->clock) {
        // position / next position follow the path and step (Human.getPos / getNextPos);
        // the next path is re-planned for the new (clock, step) and searched
        launch_plan(d, 0, s);
        launch_search(d, 0, 2, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    return MAPF_OK;
}

int mapf_gae(const float *rewards, const float *values, const float *v_last, float *adv, float *ret, int32_t T,
             int32_t M, double gamma, double lam, void *stream) {
    if (!rewards || !values || !v_last || !adv || !ret) return fail(MAPF_EINVAL, "null argument");
    if (T < 1 || M < 1) return fail(MAPF_EINVAL, "T and M must be >= 1");
    // numpy: GAMMA * next_nonterminal (python floats) then * f32 array -> f32(gamma);
    //        GAMMA * LAM * next_nonterminal -> f32(gamma * lam)   (runner.py:134-140)
    launch_gae(rewards, values, v_last, adv, ret, T, M, (float)(gamma * 1.0), (float)(gamma * lam * 1.0),
               (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_normalize_advantages(const float *ret, const float *v, const float *cret, const float *cv, float *adv_out,
                              float *cadv_out, int32_t M, double lagrange, int32_t mix, void *stream) {
    if (!ret || !v || !cret || !cv || !adv_out || !cadv_out) return fail(MAPF_EINVAL, "null argument");
    if (M < 1) return fail(MAPF_EINVAL, "M must be >= 1");
    launch_normalize(ret, v, cret, cv, adv_out, cadv_out, M, (float)lagrange, (float)(lagrange + 1.0), mix, nullptr,
                     (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_normalize_advantages_dlam(const float *ret, const float *v, const float *cret, const float *cv,
                                   float *adv_out, float *cadv_out, int32_t M, const float *lam_dev, int32_t mix,
                                   void *stream) {
    if (!ret || !v || !cret || !cv || !adv_out || !cadv_out || !lam_dev) return fail(MAPF_EINVAL, "null argument");
    if (M < 1) return fail(MAPF_EINVAL, "M must be >= 1");
    launch_normalize(ret, v, cret, cv, adv_out, cadv_out, M, 0.f, 1.f, mix, lam_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_advantage_moments(const float *ret, const float *v, const float *cret, const float *cv, int32_t M,
                           const double *mean, double *out, void *stream) {
    if (!ret || !v || !cret || !cv || !out) return fail(MAPF_EINVAL, "null argument");
    if (M < 0) return fail(MAPF_EINVAL, "M must be >= 0");
    launch_moments(ret, v, cret, cv, M, mean, out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_normalize_advantages_stats(const float *ret, const float *v, const float *cret, const float *cv,
                                    const double *stats, float *adv_out, float *cadv_out, int32_t M, double lagrange,
                                    int32_t mix, void *stream) {
    if (!ret || !v || !cret || !cv || !stats || !adv_out || !cadv_out) return fail(MAPF_EINVAL, "null argument");
    if (M < 0) return fail(MAPF_EINVAL, "M must be >= 0");
    if (M == 0) return MAPF_OK;
    launch_normalize_stats(ret, v, cret, cv, stats, adv_out, cadv_out, M, (float)lagrange, (float)(lagrange + 1.0), mix,
                           nullptr, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_normalize_advantages_stats_dlam(const float *ret, const float *v, const float *cret, const float *cv,
                                         const double *stats, float *adv_out, float *cadv_out, int32_t M,
                                         const float *lam_dev, int32_t mix, void *stream) {
    if (!ret || !v || !cret || !cv || !stats || !adv_out || !cadv_out || !lam_dev)
        return fail(MAPF_EINVAL, "null argument");
    if (M < 0) return fail(MAPF_EINVAL, "M must be >= 0");
    if (M == 0) return MAPF_OK;
    launch_normalize_stats(ret, v, cret, cv, stats, adv_out, cadv_out, M, 0.f, 1.f, mix, lam_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_episode_sum(const float *x, int32_t T, int32_t B, int32_t N, float *out, void *stream) {
    if (!x || !out) return fail(MAPF_EINVAL, "null argument");
    if (T < 0 || B < 1 || N < 1 || N > 128) return fail(MAPF_EINVAL, "need T >= 0, B >= 1, N in 1..128");
    launch_episode_sum(x, T, B, N, out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_perf_accumulate(const mapf_step_out *out, int32_t T, int32_t B, int32_t N, mapf_perf *perf, int32_t accumulate,
                         void *stream) {
    if (!out || !perf) return fail(MAPF_EINVAL, "null argument");
    if (T < 0 || B < 1 || N < 1 || N > 128) return fail(MAPF_EINVAL, "need T >= 0, B >= 1, N in 1..128");
    if (T == 0) return MAPF_OK;
    launch_perf_accumulate(step_out_of(out), T, B, N, perf, accumulate != 0, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_perf_add_host(mapf_perf *perf, int32_t N, const int8_t *status, const float *reward_total, const float *cost,
                       const float *goals_reached, int32_t shadow_goals, const float *constraints) {
    if (!perf) return fail(MAPF_EINVAL, "null argument");
    if (N < 1 || N > 128) return fail(MAPF_EINVAL, "N must be in 1..128");
    perf_add_step(*perf, N, status, reward_total, cost, goals_reached, shadow_goals, constraints);
    return MAPF_OK;
}

int mapf_sample_actions(const float *ps, int32_t ps_stride, int32_t *actions, int64_t *actions64, int32_t M,
                        uint64_t seed, uint32_t step, void *stream) {
    if (!ps || (!actions && !actions64)) return fail(MAPF_EINVAL, "null argument");
    if (M < 1 || ps_stride < 5) return fail(MAPF_EINVAL, "bad M / stride");
    launch_sample(ps, ps_stride, actions, actions64, M, seed, step, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

static int minibatch_window_ok(int64_t n, int64_t start, int64_t count, const int64_t *rows_out) {
    if (n < 1) return fail(MAPF_EINVAL, "n must be >= 1");
    if (start < 0 || count < 0) return fail(MAPF_EINVAL, "start and count must be >= 0");
    if (start > n || count > n - start) return fail(MAPF_EINVAL, "start + count must be <= n");
    if (!rows_out && count > 0) return fail(MAPF_EINVAL, "null argument");
    return MAPF_OK;
}

int mapf_minibatch_rows(uint64_t seed, uint32_t epoch, int64_t n, int64_t start, int64_t count, int64_t *rows_out,
                        void *stream) {
    if (int rc = minibatch_window_ok(n, start, count, rows_out)) return rc;
    if (count == 0) return MAPF_OK;
    launch_minibatch_rows(shuffle_key(seed, epoch, (uint64_t)n), start, count, rows_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_minibatch_rows_host(uint64_t seed, uint32_t epoch, int64_t n, int64_t start, int64_t count,
                             int64_t *rows_out) {
    if (int rc = minibatch_window_ok(n, start, count, rows_out)) return rc;
    const ShuffleKey key = shuffle_key(seed, epoch, (uint64_t)n);
    for (int64_t j = 0; j < count; ++j) rows_out[j] = (int64_t)shuffle_index(key, (uint64_t)(start + j));
    return MAPF_OK;
}

int mapf_gather_rows(const mapf_gather_spec *spec, void *stream) {
    if (!spec || !spec->rows) return fail(MAPF_EINVAL, "null argument");
    if (spec->count < 1 || spec->count > MAPF_GATHER_MAX) return fail(MAPF_EINVAL, "count must be in 1..16");
    if (spec->T < 1 || spec->B < 1 || spec->M < 1) return fail(MAPF_EINVAL, "T, B and M must be >= 1");
    GatherArgs a{};
    a.rows = spec->rows;
    a.T = spec->T;
    a.B = spec->B;
    a.count = spec->count;
    int64_t chunks = 0;
    for (int i = 0; i < spec->count; ++i) {
        const mapf_gather_array &g = spec->arrays[i];
        if (!g.src || !g.dst) return fail(MAPF_EINVAL, "null src or dst");
        if (g.row_bytes < 4 || (g.row_bytes & 3)) return fail(MAPF_EINVAL, "row_bytes must be a positive multiple of 4");
        if (((uintptr_t)g.src | (uintptr_t)g.dst) & 3) return fail(MAPF_EINVAL, "src and dst must be 4-byte aligned");
        a.nbig += g.row_bytes > GATHER_SMALL;
    }
    int nb = 0, ns = a.nbig;                       // big arrays first, each group in the caller's order
    for (int i = 0; i < spec->count; ++i) {
        const mapf_gather_array &g = spec->arrays[i];
        const bool big = g.row_bytes > GATHER_SMALL;
        const int k = big ? nb++ : ns++;
        a.src[k] = static_cast<const char *>(g.src);
        a.dst[k] = static_cast<char *>(g.dst);
        a.row_bytes[k] = g.row_bytes;
        if (!((((uintptr_t)g.src | (uintptr_t)g.dst) & 15) || (g.row_bytes & 15))) a.vec16 |= 1u << k;
    }
    for (int k = 0; k < a.nbig; ++k) {
        a.chunk_begin[k] = (int)chunks;
        chunks += (a.row_bytes[k] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (chunks > 0x7FFFFFFF) return fail(MAPF_EINVAL, "more than 2^31 - 1 workgroups");
    }
    a.chunk_begin[a.nbig] = (int)chunks;
    a.chunks_per_row = chunks > 0 ? (int)chunks : 1;
    const int64_t blocks = spec->M * a.chunks_per_row;
    if (spec->M > 0x7FFFFFFF || blocks > 0x7FFFFFFF) return fail(MAPF_EINVAL, "more than 2^31 - 1 workgroups");
    launch_gather_rows(a, blocks, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

// ---- grid symmetries (mapf_sym.h) ----
static int sym_ok(int32_t g) { return g >= 0 && g <= 7 ? MAPF_OK : fail(MAPF_EINVAL, "g must be in 0..7"); }

int mapf_sym_cell(int32_t g, int32_t F, int32_t r, int32_t c, int32_t *r2, int32_t *c2) {
    if (int rc = sym_ok(g)) return rc;
    if (!r2 || !c2) return fail(MAPF_EINVAL, "null argument");
    if (F < 1 || r < 0 || r >= F || c < 0 || c >= F) return fail(MAPF_EINVAL, "need F >= 1 and a cell (r, c) inside F x F");
    int rr, cc;
    sym_cell(g, F, r, c, rr, cc);
    *r2 = rr;
    *c2 = cc;
    return MAPF_OK;
}

int64_t mapf_sym_action(int32_t g, int64_t a) { return sym_action(g & 7, a); }

int mapf_sym_vec_host(const float *vec, int64_t n, int32_t g, float *out) {
    if (int rc = sym_ok(g)) return rc;
    if (n < 0 || ((!vec || !out) && n > 0)) return fail(MAPF_EINVAL, "null argument or n < 0");
    for (int64_t i = 0; i < n; ++i) {
        float v[4] = {vec[4 * i], vec[4 * i + 1], vec[4 * i + 2], vec[4 * i + 3]};
        sym_vec(g, v, out + 4 * i);
    }
    return MAPF_OK;
}

int mapf_sym_cols_host(const float *cols, int64_t n, int32_t g, float *out) {
    if (int rc = sym_ok(g)) return rc;
    if (n < 0 || ((!cols || !out) && n > 0)) return fail(MAPF_EINVAL, "null argument or n < 0");
    for (int64_t i = 0; i < n; ++i) {
        float v[NA];
        for (int a = 0; a < NA; ++a) v[a] = cols[NA * i + a];
        sym_cols(g, v, out + NA * i);
    }
    return MAPF_OK;
}

int mapf_sym_obs_host(const float *obs, int64_t n_agents, int32_t C, int32_t F, int32_t g, float *out) {
    if (int rc = sym_ok(g)) return rc;
    if (n_agents < 0 || C < 1 || F < 1) return fail(MAPF_EINVAL, "need n_agents >= 0, C >= 1, F >= 1");
    if ((!obs || !out || obs == out) && n_agents > 0) return fail(MAPF_EINVAL, "null argument, or out == obs");
    const int64_t FF = (int64_t)F * F;
    for (int64_t p = 0; p < n_agents * C; ++p)
        for (int i = 0; i < F; ++i)
            for (int j = 0; j < F; ++j) {
                int r, c;
                sym_cell_inv(g, F, i, j, r, c);
                out[p * FF + i * F + j] = obs[p * FF + r * F + c];
            }
    return MAPF_OK;
}

int mapf_sym_compose(int32_t g1, int32_t g2) { return sym_compose(g1 & 7, g2 & 7); }
int mapf_sym_inverse(int32_t g) { return sym_inverse(g & 7); }

static int sym_draw_ok(int64_t start, int64_t count, uint32_t allowed, const uint8_t *sym_out) {
    if (allowed == 0 || allowed > 0xFFu) return fail(MAPF_EINVAL, "allowed must be in 1..0xFF");
    if (start < 0 || count < 0) return fail(MAPF_EINVAL, "start and count must be >= 0");
    if (!sym_out && count > 0) return fail(MAPF_EINVAL, "null argument");
    return MAPF_OK;
}

int mapf_sym_draw(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed, uint8_t *sym_out,
                  void *stream) {
    if (int rc = sym_draw_ok(start, count, allowed, sym_out)) return rc;
    if (count == 0) return MAPF_OK;
    launch_sym_draw(seed, epoch, start, count, allowed, sym_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

int mapf_sym_draw_host(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed,
                       uint8_t *sym_out) {
    if (int rc = sym_draw_ok(start, count, allowed, sym_out)) return rc;
    for (int64_t j = 0; j < count; ++j) sym_out[j] = (uint8_t)sym_draw(seed, epoch, (uint64_t)(start + j), allowed);
    return MAPF_OK;
}

int mapf_gather_rows_sym(const mapf_gather_sym_spec *spec, void *stream) {
    if (!spec || !spec->rows) return fail(MAPF_EINVAL, "null argument");
    if (spec->count < 1 || spec->count > MAPF_GATHER_MAX) return fail(MAPF_EINVAL, "count must be in 1..16");
    if (spec->T < 1 || spec->B < 1 || spec->M < 1) return fail(MAPF_EINVAL, "T, B and M must be >= 1");
    const int N = spec->N, C = spec->C, F = spec->F;
    if (N < 1) return fail(MAPF_EINVAL, "N must be >= 1");
    if (F < 1 || F > 16) return fail(MAPF_EINVAL, "F must be in 1..16");
    if (C < 1 || C > 7) return fail(MAPF_EINVAL, "C must be in 1..7");
    if (spec->sym && !(F & 1)) return fail(MAPF_EINVAL, "F must be odd with sym: an even window is not centred");
    const int64_t CFF = (int64_t)C * F * F, WPA = obs_bits_words(C, F);
    SymGatherArgs a{};
    a.rows = spec->rows;
    a.sym = spec->sym;
    a.T = spec->T;
    a.B = spec->B;
    a.N = N;
    a.C = C;
    a.F = F;
    a.count = spec->count;
    for (int i = 0; i < spec->count; ++i) {
        const mapf_gather_sym_array &g = spec->arrays[i];
        if (!g.src || !g.dst) return fail(MAPF_EINVAL, "null src or dst");
        if (g.src_row_bytes < 4 || (g.src_row_bytes & 3) || g.dst_row_bytes < 4 || (g.dst_row_bytes & 3))
            return fail(MAPF_EINVAL, "src_row_bytes and dst_row_bytes must be positive multiples of 4");
        if (((uintptr_t)g.src | (uintptr_t)g.dst) & 3) return fail(MAPF_EINVAL, "src and dst must be 4-byte aligned");
        int64_t want_src = g.src_row_bytes, want_dst = g.src_row_bytes;
        switch (g.kind) {
        case MAPF_GATHER_PLAIN: break;
        case MAPF_GATHER_OBS_F32: want_src = want_dst = N * CFF * 4; break;
        case MAPF_GATHER_OBS_BITS: want_src = N * WPA * 4, want_dst = N * CFF * 4; break;
        case MAPF_GATHER_VEC: want_src = want_dst = (int64_t)N * 16; break;
        case MAPF_GATHER_ACTION32: want_src = want_dst = (int64_t)N * 4; break;
        case MAPF_GATHER_ACTION64: want_src = want_dst = (int64_t)N * 8; break;
        case MAPF_GATHER_COLS: want_src = want_dst = (int64_t)N * 4 * NA; break;
        default: return fail(MAPF_EINVAL, "kind must be one of MAPF_GATHER_* (0..6)");
        }
        if (g.src_row_bytes != want_src || g.dst_row_bytes != want_dst)
            return fail(MAPF_EINVAL, "src_row_bytes / dst_row_bytes do not match the kind and N, C, F");
        if (g.dst_row_bytes > 0x7FFFFFFF) return fail(MAPF_EINVAL, "dst_row_bytes above 2^31 - 1");
        if (g.kind == MAPF_GATHER_ACTION64 && (((uintptr_t)g.src | (uintptr_t)g.dst) & 7))
            return fail(MAPF_EINVAL, "int64 action src and dst must be 8-byte aligned");
        // the packed words staged for one piece: the agents under min(row, GATHER_CHUNK) / 4 floats
        if (g.kind == MAPF_GATHER_OBS_BITS && std::min<int64_t>(N, (GATHER_CHUNK / 4 - 1) / CFF + 2) * WPA > SYM_LDS_WORDS)
            return fail(MAPF_EINVAL, "N, C, F: a piece's packed words do not fit the staging buffer");
        a.nbig += g.dst_row_bytes > GATHER_SMALL;
    }
    int nb = 0, ns = a.nbig;                       // big arrays first, each group in the caller's order
    int64_t chunks = 0;
    for (int i = 0; i < spec->count; ++i) {
        const mapf_gather_sym_array &g = spec->arrays[i];
        const int k = g.dst_row_bytes > GATHER_SMALL ? nb++ : ns++;
        a.src[k] = static_cast<const char *>(g.src);
        a.dst[k] = static_cast<char *>(g.dst);
        a.src_row_bytes[k] = g.src_row_bytes;
        a.dst_row_bytes[k] = g.dst_row_bytes;
        a.kind[k] = g.kind;
        // 16-byte accesses: the destination always; the source too where its bytes are copied
        uintptr_t bits = (uintptr_t)g.dst | (uintptr_t)g.dst_row_bytes;
        if (g.kind != MAPF_GATHER_OBS_BITS) bits |= (uintptr_t)g.src | (uintptr_t)g.src_row_bytes;
        if (!(bits & 15)) a.vec16 |= 1u << k;
    }
    for (int k = 0; k < a.nbig; ++k) {
        a.chunk_begin[k] = (int)chunks;
        chunks += (a.dst_row_bytes[k] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (chunks > 0x7FFFFFFF) return fail(MAPF_EINVAL, "more than 2^31 - 1 workgroups");
    }
    a.chunk_begin[a.nbig] = (int)chunks;
    a.chunks_per_row = chunks > 0 ? (int)chunks : 1;
    const int64_t blocks = spec->M * a.chunks_per_row;
    if (spec->M > 0x7FFFFFFF || blocks > 0x7FFFFFFF) return fail(MAPF_EINVAL, "more than 2^31 - 1 workgroups");
    launch_gather_rows_sym(a, blocks, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return MAPF_OK;
}

}  // extern "C"
