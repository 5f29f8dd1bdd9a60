/*
 * include/mapf.h -- C ABI of libmapf.so, the MI355X-native batched MAPF env.
 *
 * Drop-in boundary for the reference's per-step env API.
 * The reference (Nielsencu/primal-ppo) has no FFI layer: its boundary is the
 * Python method API of mapf_gym.MapfGym, called by runner.py:30-100 and
 * evaluate.py:218-269 in this fixed order:
 *
 *   MapfGym() / FixedMapfGym(...)   mapf_gym.py:164-173 / :648-669  -> mapf_reset
 *   getAllObservations()            mapf_gym.py:327-336             -> mapf_observe
 *   getActionStatus(a)              mapf_gym.py:434-480             -> mapf_step (status)
 *   calculateActionReward(a, st)    mapf_gym.py:483-511             -> mapf_step (reward, shadow_goals)
 *   calculateCostReward(a)          mapf_gym.py:528-533             -> mapf_step (cost)
 *   getTrainValid(a)                mapf_gym.py:535-550             -> mapf_step (train_valid)
 *   jointStep(a, st)                mapf_gym.py:614-637             -> mapf_step (MAPF_STEP_COMMIT)
 *   jointStep + getAllObservations  runner.py:84-97                 -> mapf_step_observe (one launch)
 *   agent.bfsMap / makeBfsMap       mapf_gym.py:211-244             -> mapf_bfs
 *   renderWorld / MapfGym._render   util.py:189-232, mapf_gym.py:639 -> mapf_render
 *   Runner.run GAE                  runner.py:117-149               -> mapf_gae
 *   Model.train normalisation       model.py:106-113                -> mapf_normalize_advantages
 *   Model.imitation_train           model.py:205-231                -> mapf_imitation_loss
 *   Model.step sampling             model.py:38-40                  -> mapf_sample_actions
 *   minibatch shuffle + indexing    driver.py:123-134               -> mapf_minibatch_rows, mapf_gather_rows
 *
 * Conventions
 *  - One handle = B lockstep environments resident on one GPU (Structure of
 *    Arrays in HBM).  The handle owns its device state; the caller owns every
 *    output buffer (device pointers, e.g. torch tensors' data_ptr()).
 *  - Calls are asynchronous on the caller's HIP stream (`stream` is a
 *    hipStream_t passed as void*; NULL = the null stream).  A handle is not
 *    thread-safe: one handle per GPU / process.
 *  - Errors: 0 = OK, negative = error code (MAPF_E*); mapf_last_error() gives
 *    a message (thread-local).  Impossible states the reference raises on
 *    (mapf_gym.py:456,508,588,610; astar_4.py:109) are counted on the device
 *    (mapf_get_counters) instead of raised.
 *  - No C++ exceptions cross this boundary.
 */
#ifndef MAPF_H
#define MAPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAPF_ABI_VERSION 1

#define MAPF_OK 0
#define MAPF_EINVAL (-1)
#define MAPF_EDEVICE (-2)
#define MAPF_ENOMEM (-3)
#define MAPF_ESTATE (-4)

/* Environment configuration.  Field names follow alg_parameters.py
 * (EnvParameters :27-48, TrainingParameters :76-78, NetParameters :103-104). */
typedef struct mapf_config {
    int32_t num_envs;        /* B: environments on this device                     */
    int32_t num_agents;      /* N: EnvParameters.N_AGENTS, 1..64                    */
    int32_t height, width;   /* H, W: grid, 1..128 each                             */
    int32_t fov;             /* F: EnvParameters.FOV_SIZE, 1..16                    */
    int32_t num_channel;     /* C: 5, 6 (NetParameters.NUM_CHANNEL) or 7 (+BFS ch) */
    int32_t use_da, use_hp;  /* FixedMapfGym(useDA, useHP), mapf_gym.py:662-663    */
    int32_t lifelong;        /* EnvParameters.LIFELONG                              */
    int32_t human_mode;      /* 0 LoopingHuman, 1 Human (random goals), 2 FixedPathHuman */
    int32_t goal_mode;       /* 0 agentsSequence (FixedMapfGym), 1 getFreeCell (MapfGym) */
    int32_t fix_choice;      /* fixActions random.choice: 0 rotating rule, 1 Philox */
    int32_t shared_map;      /* 1: one H x W map for all envs, 0: one map per env    */
    int32_t keep_bfs;        /* maintain agent.bfsMap (makeBfsMap) for every agent   */
    int32_t max_seq;         /* S: agentsSequence capacity per agent (goal_mode 0)  */
    int32_t max_human_seq;   /* human pose sequence capacity (human_mode 2)          */
    int32_t k_predict;       /* TrainingParameters.K_TIMESTEP_PREDICT                */
    int32_t penalty_radius;  /* EnvParameters.PENALTY_RADIUS                         */
    float action_cost;       /* EnvParameters.ACTION_COST                            */
    float collision_cost;    /* EnvParameters.COLLISION_COST                         */
    float human_collision_cost; /* EnvParameters.HUMAN_COLLISION_COST                */
    float repeat_cost;       /* EnvParameters.REPEAT_POS                             */
    float goal_reward;       /* EnvParameters.GOAL_REWARD (runner.py:89-91)          */
    int32_t env_offset;      /* global index of env 0 (RNG counters; sharding)       */
    uint32_t reserved;
    uint64_t seed;           /* Philox key (SetupParameters.SEED)                    */
} mapf_config;

typedef struct mapf_env mapf_env;

/* Reset specification.  All pointers are HOST pointers.
 * mode 0 (FixedMapfGym, mapf_gym.py:648-669): maps + agent sequences +
 *   human start/goal (LoopingHuman) or human pose sequence (FixedPathHuman).
 * mode 1 (MapfGym, mapf_gym.py:164-184): maps + Philox draws for the human
 *   entrance/goal and agent starts/goals (getFreeCell semantics). */
typedef struct mapf_reset_spec {
    int32_t mode;
    int32_t reserved;
    const int8_t *maps;          /* [shared_map ? 1 : B][H][W], values 0 (free) / -1 (obstacle) */
    const int32_t *seq;          /* [B][N][S][2] (row, col)                    mode 0 */
    const int32_t *seq_len;      /* [B][N], 1..S                               mode 0 */
    const int32_t *human_start;  /* [B][2]                                     mode 0, human_mode 0 */
    const int32_t *human_goal;   /* [B][2]                                     mode 0, human_mode 0 */
    const int32_t *human_seq;    /* [B][max_human_seq][2]                      human_mode 2 */
    const int32_t *human_seq_len;/* [B], 2..max_human_seq                      human_mode 2 */
    uint64_t seed;               /* mode 1: overrides config.seed when non-zero */
} mapf_reset_spec;

/* Per-step outputs: DEVICE pointers owned by the caller; NULL = not written. */
typedef struct mapf_step_out {
    int8_t *status;          /* [B][N]  getActionStatus: 1, -1, -2, -3, -4          */
    float *reward;           /* [B][N]  calculateActionReward (before GOAL_REWARD)   */
    int32_t *shadow_goals;   /* [B]     calculateActionReward's shadowGoal           */
    float *cost;             /* [B][N]  calculateCostReward                          */
    float *train_valid;      /* [B][N][5] getTrainValid                              */
    int32_t *actions_fixed;  /* [B][N]  actions after fixActions                      */
    float *goals_reached;    /* [B][N]  jointStep's goalsReached                      */
    float *constraints;      /* [B][N]  jointStep's constraintsViolated               */
    float *reward_total;     /* [B][N]  reward + GOAL_REWARD where goal reached (runner.py:89-91) */
} mapf_step_out;

#define MAPF_STEP_COMMIT 1u  /* apply jointStep (move, goals, human, counters).  Without it
                                only the pre-step outputs are produced and no state changes. */

/* Host-side snapshot of the env state (checkpoint / test hook).  Any pointer
 * may be NULL (skipped).  Cells are (row, col). */
typedef struct mapf_state {
    int32_t *pos;            /* [B][N][2]                                  */
    int32_t *goal;           /* [B][N][2]                                  */
    int32_t *last_action;    /* [B][N]   -1 = none (reset)                 */
    int32_t *seq_cursor;     /* [B][N]   util.Sequence.curIdx              */
    int32_t *human;          /* [B][10]  pos r,c; next r,c; goal r,c; step; path len; entrance r,c */
    int32_t *human_path;     /* [B][path_capacity][2]                      */
    uint32_t *clock;         /* [B]      steps since reset                 */
} mapf_state;

const char *mapf_last_error(void);
int mapf_abi_version(void);

int mapf_create(const mapf_config *cfg, int device, mapf_env **out);
int mapf_destroy(mapf_env *env);
int mapf_path_capacity(const mapf_env *env);       /* human path capacity per env */
/* 1 if mapf_step_observe runs as ONE launch for this configuration (N <= 8,
 * no BFS channel, no scripted human), 0 if it runs as step + observe. */
int mapf_step_observe_fused(const mapf_env *env);

int mapf_reset(mapf_env *env, const mapf_reset_spec *spec, void *stream);

/* Obstacle maps generated on the device, then a seeded reset on them (mode 1 of
 * mapf_reset) -- no host maps, no upload, asynchronous on `stream`.
 *   MAPF_MAPS_WAREHOUSE: MapfGym()'s map (mapf_gym.py:166 -> generateWarehouse(num_block=
 *     [lo, hi]), map_generator.py:127-138): per env (one map if shared_map) a length L
 *     uniform in [lo, hi], breadth int(L / (2/3)), shelves as the reference places them
 *     (bit-exact for a given L), at the top-left of the H x W stack, the rest obstacles.
 *     Needs H >= hi, W >= int(hi / (2/3)).
 *   MAPF_MAPS_RANDOM: random_generator's rule -(rand < p) (map_generator.py:23) over H x W,
 *     p = density.
 *   largest = 1: free cells outside the largest 4-connected free component become
 *     obstacles (H * W <= 8192).
 * Draws: Philox (key = seed, or config.seed if 0; counters (env id, 10, epoch, k)).
 * maps_out: optional DEVICE int8 [shared_map ? 1 : B][H][W] copy of the maps. */
#define MAPF_MAPS_WAREHOUSE 0
#define MAPF_MAPS_RANDOM 1
typedef struct mapf_mapgen_spec {
    int32_t kind;            /* MAPF_MAPS_*                                    */
    int32_t lo, hi;          /* warehouse length range (EnvParameters.WORLD_SIZE) */
    int32_t largest;         /* keep the largest 4-connected free component   */
    float density;           /* random maps: obstacle probability             */
    uint32_t epoch;          /* draw epoch (e.g. the rollout index)           */
    uint64_t seed;           /* 0: config.seed                                */
} mapf_mapgen_spec;
int mapf_reset_generated(mapf_env *env, const mapf_mapgen_spec *spec, int8_t *maps_out, void *stream);

/* One lockstep step for all B envs: actions are DEVICE int32 [B][N] in 0..4. */
int mapf_step(mapf_env *env, const int32_t *actions, const mapf_step_out *out, uint32_t flags, void *stream);

/* Env-only benchmark / random-policy rollouts: draw the uniform random policy's
 * actions on the device (same Philox stream as mapf_random_actions), write them
 * to actions_out (DEVICE int32 [B][N]) and step with them, in one launch. */
int mapf_step_random(mapf_env *env, int32_t *actions_out, const mapf_step_out *out, uint32_t flags, void *stream);

/* getAllObservations for all envs: obs DEVICE float [B][N][C][F][F], vec [B][N][4]. */
int mapf_observe(mapf_env *env, float *obs, float *vec, void *stream);

/* jointStep + getAllObservations in ONE launch (runner.py:84-97 calls them back
 * to back): the committed step of mapf_step followed by mapf_observe, identical
 * outputs.  Each workgroup steps its envs and observes them from LDS; the
 * previous step's search work rides in the same launch (its results are next
 * needed two steps later).  Configurations the fused kernel does not cover
 * (N > 8, scripted humans, the BFS channel, very large maps) run the two
 * launches.  mapf_step_observe_random draws the random policy like
 * mapf_step_random. */
int mapf_step_observe(mapf_env *env, const int32_t *actions, const mapf_step_out *out, float *obs, float *vec,
                      void *stream);
int mapf_step_observe_random(mapf_env *env, int32_t *actions_out, const mapf_step_out *out, float *obs,
                             float *vec, void *stream);

/* Random-policy rollout: T x (mapf_step_observe_random), i.e. runner.py:64-100
 * with the uniform random policy T times, in ONE launch where the configuration
 * allows (mapf_rollout_random_fused; otherwise T launches) -- identical results.
 * slots = 1: step t writes slot t of [T]-leading DEVICE buffers (actions_out
 * [T][B][N], every out field [T][...], obs [T][B][N][C][F][F], vec [T][B][N][4]),
 * i.e. rollout buffers; slots = 0: every step overwrites the same [B]-leading
 * buffers.  Each wave of the one-launch kernel owns one env and loops step ->
 * observe -> its own search work, so steps overlap other envs' store drains.
 *
 * `slots` is a bit set.  MAPF_SLOTS (bit 0) is the meaning above.
 * MAPF_SLOTS_BAND_CLEAN (bit 1) is a promise by the caller: the config-static
 * zero band of every slot passed (channel 5 of every agent while use_hp is off:
 * floats [5*F*F, 6*F*F) of each [C][F][F] block, 0.0 at every step) already
 * holds zeros -- typically because an earlier launch of this handle wrote these
 * very slots without the bit and nothing else has written them since.  The
 * pair-lane kernel (mapf_rollout_random_fused == 1) then leaves out the stores
 * that lie wholly inside the band, in aligned pieces (mapf_obs_band_skip gives the
 * exact set): at c2 2,577 of 3,001 bytes per agent-step are written.  Every
 * other byte, and every other output, is written as without the bit.  The bit
 * is ignored -- everything is stored -- where no such band exists (use_hp on,
 * num_channel < 6, fov > 11), without MAPF_SLOTS, and in the one-wave-per-env
 * and per-step forms.  The library keeps no record of buffers: an address says
 * nothing about its content, so only the caller can make this promise. */
#define MAPF_SLOTS 1
#define MAPF_SLOTS_BAND_CLEAN 2
/* MAPF_SLOTS_OBS_BITS (bit 2), on mapf_rollout_random / _actions / _descent: `obs` points at the
 * packed observation buffer uint32 [T or 1][B][N][WPA] ("Packed observations" below) instead of
 * float [T or 1][B][N][C][F][F]; every other buffer is unchanged.  Orthogonal to MAPF_SLOTS.  With it
 * MAPF_SLOTS_BAND_CLEAN is ignored (packed zeros cost nothing to write), and the mapf_rollout_*plan
 * texts carry ",bits" inside the angle brackets. */
#define MAPF_SLOTS_OBS_BITS 4
int mapf_rollout_random(mapf_env *env, int32_t T, int32_t slots, int32_t *actions_out, const mapf_step_out *out,
                        float *obs, float *vec, void *stream);
/* Which kernel mapf_rollout_random runs for this configuration (0: T per-step
 * launches).  1: the pair-lane kernel -- N in 5..8 with a whole number of float4s
 * per env's observation, one shared map whose padded bitmap fits 64 words
 * (W + 2*(F/2) <= 32, H + 2*(F/2) <= 64), no BFS channel, Human or LoopingHuman,
 * random (MapfGym) goals.  2: the one-wave-per-env kernel -- every other
 * configuration whose per-env LDS (map rows, observation bit-stream, BFS image)
 * fits 64 KiB: up to 64 agents, per-env maps, the BFS channel (c4, c5). */
int mapf_rollout_random_fused(const mapf_env *env);
/* The stores a MAPF_SLOTS_BAND_CLEAN launch leaves out, computed on the host (no device call) by
 * the function the kernel runs: for one env whose observation slice [N][C][F][F] starts at byte
 * address byte_offset (a multiple of 16; only its value modulo the unit matters), skip[q] = 1 iff
 * float4 q of the slice is not stored, for q < min(n, float4s per env).  A float4 is skipped iff
 * the unit-aligned `unit` bytes around it (16, 64 or 128) lie wholly inside one agent's zero band.
 * unit = 0: the unit the kernel uses (64).  For units above 16 the set depends on the slice's
 * address: pass the address of the very slot and env asked about, obs + ((t * B + b) * N*C*F*F) * 4.
 * Returns the float4s per env, or a negative error. */
int mapf_obs_band_skip(const mapf_config *cfg, int32_t unit, uint64_t byte_offset, uint8_t *skip, int32_t n);
/* Sparse slot-buffer rollouts: store only the observation pieces that change.  The policy's rollout
 * (policy 0 random, 1 the caller's tape in `actions`, 2 descent, 3 pibt; as mapf_rollout_random /
 * _actions / _descent / _pibt with slots = MAPF_SLOTS) over rollout buffers that are used again and
 * again.  Every observation float is 0.0 or 1.0 and most are 0.0; a piece is 16 consecutive floats
 * (64 bytes) of an env's [N][C][F][F] slice in one slot.
 *   shadow  DEVICE uint32 [T][B][16], 64-byte aligned, the caller's: bit p of an env-slot's 16 words
 *           is 1 iff piece p of that env in that slot holds a non-zero float.
 *   valid   the promise, as MAPF_SLOTS_BAND_CLEAN's: for every slot t < valid the shadow says what
 *           `obs` holds now (typically: an earlier mapf_rollout_sparse wrote these slots with this
 *           shadow and nothing else has written `obs` or the shadow since).  0 promises nothing.
 * For t < valid the launch stores exactly the pieces that the shadow names or that hold a non-zero
 * now; for t >= valid it stores every float.  Either way it writes the slot's new shadow, and `obs`,
 * like every other output, ends byte for byte as after a mapf_rollout_random with MAPF_SLOTS -- as
 * long as the promise holds.  Whoever writes `obs` in between (another library, a raw pointer) passes
 * valid = 0 next time.  The library keeps no record of buffers.
 * The form takes effect in the pair-lane kernel where an env's slice is a whole number of pieces and
 * `obs` is 64-byte aligned (mapf_obs_sparse_applies: N = 8 with an even channel count).  Elsewhere the
 * shadow is neither read nor written and the launch is the MAPF_SLOTS one, with MAPF_SLOTS_BAND_CLEAN
 * if valid >= T.  mapf_rollout_sparse_plan: the launch's form as text, as mapf_rollout_plan; the sparse
 * form reads e.g. "rollout_random_kernel<true,4,sparse64>". */
int mapf_rollout_sparse(mapf_env *env, int32_t policy, int32_t T, int32_t *actions, const mapf_step_out *out,
                        float *obs, float *vec, uint32_t *shadow, int32_t valid, void *stream);
int mapf_rollout_sparse_plan(const mapf_env *env, int32_t policy, const float *obs, char *buf, int32_t n);
/* Host only: 1 if the sparse form applies to this configuration with `obs` at this address, else 0
 * (negative on error). */
int mapf_obs_sparse_applies(const mapf_config *cfg, uint64_t obs_address);
/* The pacing gate of the grouped pair-lane kernel (roll_group with roll_slack >= 0), computed on the
 * host (no device call) by the function the kernel runs.  The `live` waves of a workgroup (1..64, those
 * that own an env) share a ring of 16 counters; a wave that has finished step t adds 1 to counter
 * t % 16.  A wave may start step t (>= 0) once *word has reached *target.  Returns 1 with the two set,
 * 0 if step t needs no wait at all (t <= slack), or a negative error.  slack >= 0; more than 14 is
 * paced as 14. */
int mapf_pace_gate(int32_t t, int32_t slack, int32_t live, int32_t *word, uint32_t *target);
/* LDS bytes the mapf_observe launch requests with `obs_envs` envs per workgroup (0: the default
 * rule, 64 / N for N <= 8 else 1, at most num_envs), computed on the host (no device call) by the
 * functions the launch and mapf_create / mapf_set_tuning run.  The request is the observing workgroup's
 * own LDS or, where the launch may host the step's searches (W <= 32, H <= 64) and that is more, the
 * four search waves'.  If max_lds > 0 and envs_out != NULL, *envs_out = the envs per workgroup the
 * library uses under that limit: the largest count up to the requested one whose request fits (0, and
 * MAPF_EINVAL, if not even one env fits: mapf_create refuses such a configuration on such a device).
 * With max_lds = 0 nothing is fitted and *envs_out is the requested count.
 * Returns the bytes of THAT choice when max_lds > 0, of the requested one otherwise; negative on error. */
int64_t mapf_observe_lds(const mapf_config *cfg, int32_t obs_envs, int32_t max_lds, int32_t *envs_out);

/* Launch tuning of one handle: which form of a kernel the launches take (the measured choices
 * of DESIGN.md §4 / §9).  The reference has no counterpart (its env is Python); these fields
 * only pick between forms that produce identical results.  mapf_create sets the defaults
 * (mapf_tuning_default); nothing is read from the process environment.  A field at its
 * default means "the measured choice for this configuration", which may depend on B, N, the
 * map size, slots and the device (CU count, LDS size, the kernels' VGPR counts).
 * mapf_rollout_perf's kernels store nothing per step, so the fields that manage store drains do not
 * apply to them: they honour roll_occ (pair-lane: the LDS request per workgroup), wide_grid (0: the
 * agent loop) and xcd_remap, and ignore roll_group, roll_fair, roll_slack and every other wide_* field
 * (always one wave per env, one env per workgroup, the neighbour grid sharing the search's LDS area,
 * no pacing, no priority).  Their LDS holds the map rows, the search scratch, the path copies and the
 * policy's rows only. */
typedef struct mapf_tuning {
    /* pair-lane rollout (mapf_rollout_random_fused == 1: N in 5..8, shared map) */
    int32_t roll_occ;        /* workgroups per CU the LDS request admits: 0 = ceil(grid / CUs), 1..16      */
    int32_t roll_group;      /* the 16 waves of a CU in one workgroup: -1 auto (slots, or roll_fair > 0), 0, 1 */
    int32_t roll_fair;       /* grouped, issue priority by progress: -1 auto (4 in place and sparse, 0 slots), 0 off, n */
    int32_t roll_slack;      /* grouped, roll_fair 0: waves paced within n steps of the slowest (< 0 off;
                                more than 14 paces as 14: mapf_pace_gate)                                 */
    /* one-wave-per-env rollout (mapf_rollout_random_fused == 2: up to 64 agents, per-env maps, C = 7) */
    int32_t wide_nt;         /* nontemporal observation stores: -1 auto (slots, or a [B] buffer > 128 MB), 0, 1 */
    int32_t wide_pipe;       /* 1 auto: a stepping and observing waves per env where they fit; 0 one wave   */
    int32_t wide_grid;       /* 1 auto: the step's LDS neighbour grid where it fits; 0 the agent loop       */
    int32_t wide_overlap;    /* 1 auto: pipelined through LDS counters (no BFS channel); 0 per-step barriers */
    int32_t wide_obs;        /* observing waves per env in the overlapped form: 2 (auto, where they fit) or 1 */
    int32_t wide_epw;        /* envs per workgroup: 0 auto (all the envs of a CU where the form allows), n    */
    int32_t wide_pair;       /* epw > 1: 0 wave w is env w / wpe's role w % wpe, 1 env w % epw's role w / epw */
    int32_t wide_slack;      /* one wave per env, epw > 1: paced within n steps of the group's slowest (< 0 off) */
    int32_t wide_fair;       /* one wave per env, epw > 1: issue priority by progress instead of waits (0 off) */
    int32_t wide_prio;       /* pipelined: the stepping wave issues at priority 3 (0 off)                   */
    int32_t wide_bfsobs;     /* three-wave form: the observers search the rebuilt BFS maps (0: the stepper)  */
    int32_t xcd_remap;       /* persistent kernels: XCD-aware env order (0 off)                            */
    /* per-step launches */
    int32_t obs_envs;        /* envs per observe workgroup: 0 auto (64 / N for N <= 8, else 1, reduced until
                                the launch's LDS fits the device: mapf_observe_lds), 1..64 (at most B; a value
                                whose LDS does not fit is refused, the message names the largest that does)  */
    int32_t step_block;      /* threads per step workgroup: 64, 128 or 256                                 */
    int32_t search_blocks;   /* workgroups of an observe launch that run search work: 1..1024              */
    int32_t band_blocks;     /* zero-band workgroups of the fused step+observe launch: 0..4096             */
    int32_t agent_lanes;     /* 1: the agent-per-lane step kernel even for N <= 8 (no pair-lane kernels)    */
    int32_t serial_search;   /* 1: wide maps search, then observe, on one stream                           */
    int32_t no_defer;        /* 1: a forked search is joined inside its own call                           */
    int32_t diag_exp;        /* -DMAPF_STAMPS builds only: phase experiment (0 = none)                     */
} mapf_tuning;
void mapf_tuning_default(mapf_tuning *t);
int mapf_get_tuning(const mapf_env *env, mapf_tuning *t);
/* Validates every field (MAPF_EINVAL, nothing changed, on a bad one); takes effect at the next launch. */
int mapf_set_tuning(mapf_env *env, const mapf_tuning *t);
/* The kernel mapf_rollout_random would launch now for `slots`, as text into buf (n bytes, NUL-terminated),
 * e.g. "rollout_wide3_kernel<u64,1,false> wpe=3 epw=4 grid=1 overlap=1 slack=-1 fair=0".  Returns
 * mapf_rollout_random_fused's kind (0: per-step launches, text "step_observe") or a negative error.
 * `slots` takes mapf_rollout_random's bits: where MAPF_SLOTS_BAND_CLEAN takes effect the pair-lane
 * kernel's name reads e.g. "rollout_random_kernel<true,4,band64>"; the text for 0 and 1 is as before. */
int mapf_rollout_plan(const mapf_env *env, int32_t slots, char *buf, int32_t n);

/* T x mapf_step_observe(actions_in + t*B*N, ...): the caller's policy, T steps, ONE launch where
 * mapf_rollout_random_fused says so (same kernels, same coverage), otherwise T per-step launches --
 * identical results.  actions_in: DEVICE int32 [T][B][N], read-only, always [T]-leading whatever
 * `slots` says; values outside 0..4 are counted (the bad-action counter) and played as 0, exactly
 * as mapf_step does.  slots / out / obs / vec and MAPF_SLOTS_BAND_CLEAN: as mapf_rollout_random.
 * actions_fixed (out) is what was executed.  The tape is read by the launch, on the stream, not by
 * the call; it must not overlap out->actions_fixed (MAPF_EINVAL).  T = 0 does nothing.  Like
 * mapf_rollout_random the call allocates, copies and waits for nothing and may be captured (the
 * three-wave form takes an argument slot, mapf_release_captures). */
int mapf_rollout_actions(mapf_env *env, int32_t T, int32_t slots, const int32_t *actions_in,
                         const mapf_step_out *out, float *obs, float *vec, void *stream);
/* mapf_rollout_plan for mapf_rollout_actions: the same text with ",tape" inside the angle brackets,
 * e.g. "rollout_random_kernel<true,4,band64,tape>", "rollout_wide3_kernel<u64,1,true,tape>".  The
 * pair-lane kernel stages tape_k steps of an env's actions in LDS; where that does not fit the
 * grouped form the text says ungrouped=tape_lds, and where it does not fit at all the
 * one-wave-per-env kernel runs (kind 2). */
int mapf_rollout_actions_plan(const mapf_env *env, int32_t slots, char *buf, int32_t n);

/* The descent policy, T steps: independent shortest-path followers, every agent one step down
 * its own agent.bfsMap (mapf_descent_actions has the rule) -- the heuristic baseline a learned
 * policy is compared with, and the rollout kernels' cost where goals change often.  ONE launch
 * where mapf_rollout_random_fused says so (the same kernels' descent instantiations picking the
 * actions in-kernel from the tiled maps), otherwise T x (mapf_descent_actions,
 * mapf_step_observe) -- identical results.  actions_out receives the chosen actions; slots /
 * actions_out / out / obs / vec and MAPF_SLOTS_BAND_CLEAN: as mapf_rollout_random.  Requires
 * keep_bfs (MAPF_ESTATE otherwise).  T = 0 does nothing.  Like mapf_rollout_random the call
 * allocates, copies and waits for nothing and may be captured. */
int mapf_rollout_descent(mapf_env *env, int32_t T, int32_t slots, int32_t *actions_out,
                         const mapf_step_out *out, float *obs, float *vec, void *stream);
/* mapf_rollout_plan for mapf_rollout_descent: the same text with ",descent" inside the angle
 * brackets, e.g. "rollout_random_kernel<true,4,descent>", "rollout_wide3_kernel<u64,1,true,descent>".
 * The pair-lane text ends with the way the map cells are fetched (fetch=load) and, where the
 * hand-over row does not fit the grouped form's LDS, ungrouped=descent_lds.  The wide three-wave
 * form always says bfsobs=0: the stepping wave searches the maps it reads (wide_bfsobs is
 * ignored).  Kind 0: "descent_actions+step_observe", the per-step launches. */
int mapf_rollout_descent_plan(const mapf_env *env, int32_t slots, char *buf, int32_t n);

/* Launch the search work a committed step left pending (agent.bfsMap updates, the
 * humans' next paths) on its own; mapf_observe otherwise runs it inside the
 * observation launch.  Any later call that needs it flushes implicitly.
 * Also joins, on `stream`, the searches that wide maps (the split path) defer onto a
 * second stream: call it on an uncaptured stream before beginning a hipGraph capture
 * of a handle that stepped outside the capture -- a call inside the capture that would
 * have to wait for such a search fails with MAPF_ESTATE instead (a graph cannot depend
 * on work recorded before its capture began). */
int mapf_flush(mapf_env *env, void *stream);

/* Return every argument slot that captured persistent launches of this handle took (16 per
 * handle; a capture past them fails with MAPF_ESTATE and launches nothing).  The store of a
 * launch's argument block is captured with the launch, so every replay re-writes its block
 * (stream-ordered) before its kernel reads it: a graph captured before the release still replays
 * right on its own.  What the release allows is a later capture sharing that slot -- replays of the
 * two graphs must then not overlap in time (two streams at once), or one kernel may read the other's
 * block.  Safest: call it once the graphs holding this handle's captured launches are destroyed. */
int mapf_release_captures(mapf_env *env);

/* Uniform random policy (Philox, counter = env clock): DEVICE int32 [B][N]. */
int mapf_random_actions(mapf_env *env, int32_t *actions, void *stream);

/* The descent policy's actions for the current state: DEVICE int32 [B][N] (requires keep_bfs,
 * MAPF_ESTATE otherwise; flushes pending search work first, as mapf_observe does).  Agent i of an
 * env at clock t (steps since reset), D = its agent.bfsMap, own = D[pos]: S = the moves k in 1..4
 * whose target cell is inside the map with 0 <= D[target] < own (the BFS channel's rule); the
 * action is 0 if own <= 0 (at the goal, or the goal unreachable) or S is empty, else
 * mapf_descent_pick(S, t, i).  Other agents and the human are ignored: the step resolves what
 * that causes, as for any caller's actions. */
int mapf_descent_actions(mapf_env *env, int32_t *actions, void *stream);
/* The pick among the descent moves, on the host (the function the kernels run): descent_mask bit
 * k (1..4) = move k is in S; returns the first k = 1 + ((k0 + m) & 3), m = 0..3, in S, where
 * k0 = (clock + agent) & 3 -- the rotation keeps two agents from making the same tie-break
 * forever -- or 0 if S is empty.  Bits other than 1..4 are ignored. */
int mapf_descent_pick(uint32_t descent_mask, uint32_t clock, int32_t agent);

/* The PIBT policy (priority inheritance with backtracking, Okumura et al.): a one-step planner over
 * the agents' BFS maps that never produces a vertex or a swap conflict -- the collision-free
 * baseline a learned policy is compared with.  Per env at clock t (steps since reset), agents
 * i = 0..N-1 at cells p_i with goals g_i, D_i = agent.bfsMap, the human at h with next cell hn:
 *   1. Age (policy-owned state of the handle, never touched by a step): per agent a packed goal
 *      `seen` and a clock `since`.  At a pick, if since_i > t or seen_i != g_i then seen_i = g_i,
 *      since_i = t; age_i = t - since_i.  Every reset, and mapf_set_state, sets since to 0xFFFFFFFF
 *      (mapf_get_state does not export the ages: a restored state starts them anew).  Picking
 *      twice at the same clock changes nothing the second time.
 *   2. Candidates: action a in 0..4 with target q = p_i + d(a) is admitted iff the step would give
 *      it neither status -1 nor -2: q inside the map and free, q != hn, and not (p_i == hn and
 *      q == h).  C_i = the admitted actions in ascending mapf_pibt_key(dist', a, t, i), where
 *      dist = D_i[q] and, with the handle's human weight w in 0..16 (mapf_set_pibt_human_weight; 0
 *      by default), its human horizon K in 1..8 (mapf_set_pibt_human_horizon; 1 by default) and
 *      R = penalty_radius:
 *        the human's predicted cells, where it stands on path[s] of its current path of L cells:
 *          P_1 = hn, whatever the path situation; P_j = path[s + j] for j = 2..K where
 *          s + j <= L - 1 -- past the path's end there is no cell, and the path that follows is not
 *          consulted (its search may still be running);
 *        d2_j = |q - P_j|^2 in cells;
 *        level(R, d2) = 0 if d2 > constr_d2(R), else R - floor(sqrt(d2)), constr_d2(R) = the largest
 *          d2 with (R - sqrt(d2)) / R >= 0.01 in fp64 (24 for R = 5): level(R, d2_1) >= 1 exactly where
 *          an agent that ends the step on q is counted in `constraints` -- hn is the human's cell
 *          after the step --, one more per cell nearer the human, as the cost reward rises; for
 *          j >= 2 the same of the step j - 1 steps later, had the agent stayed on q;
 *        dist' = dist if dist < 0 (unreachable stays 0x7FFF), else
 *          min(dist + w * max_j level(R, d2_j), 0x7FFE), the maximum over the cells that exist.
 *      Staying (a = 0) is priced at the agent's own cell like any other target.  With w = 0,
 *      dist' = dist at any K; with K = 1 the price is that of hn alone.  Weight and horizon only
 *      reorder the admitted actions: admission, the ages and the solve do not depend on them.
 *   3. Solve: next_i undecided for all agents; in the order (age descending, index ascending)
 *      every still undecided agent calls PIBT(i, none):
 *        PIBT(i, parent): for (a, q) in C_i:
 *            skip if some k has next_k == q (vertex), or parent != none and q == p_parent (swap);
 *            next_i = q, act_i = a;
 *            if an undecided agent k != i stands on q and PIBT(k, i) fails: continue (backtrack);
 *            return true
 *          next_i = p_i, act_i = 0, return false      (a failed pick: stay, whatever the human does)
 *      Every agent is entered at most once and at most 5 N candidates are examined; the loops stop
 *      after 6 N examinations (never reached), every agent without a final pick then stays.
 * Under these actions no agent gets status -1 or -3, status -2 only goes to an agent whose pick
 * failed while it stands on hn, and in an env-step without a -2 actions_fixed equals the actions.
 *
 * mapf_pibt_actions: the policy's actions for the current state, DEVICE int32 [B][N] (requires
 * keep_bfs, MAPF_ESTATE otherwise; flushes pending search work first, as mapf_observe does);
 * updates the age arrays. */
int mapf_pibt_actions(mapf_env *env, int32_t *actions, void *stream);
/* The candidate key, on the host (the function the kernels run): cost * 8 + rank, cost = dist if
 * dist >= 0 else 0x7FFF, rank = 0 for action 0 and 1 + ((action - 1 - k0) & 3) for the moves,
 * k0 = (clock + agent) & 3 (the descent policy's rotation).  The five keys of one agent are
 * distinct. */
int mapf_pibt_key(int32_t dist, int32_t action, uint32_t clock, int32_t agent);
/* The human weight w of step 2: MAPF_EINVAL on a null env or a weight outside 0..16, and nothing
 * changes then.  No device call; the weight is an argument of the next mapf_pibt_actions /
 * mapf_rollout_pibt launch.  A captured launch keeps the weight it was captured with (its
 * argument block is stored at capture): set the weight before capturing.  Resets and
 * mapf_set_state do not touch it. */
int mapf_set_pibt_human_weight(mapf_env *env, int32_t weight);
/* The handle's human weight, or MAPF_EINVAL on a null env. */
int mapf_get_pibt_human_weight(const mapf_env *env);
/* The human horizon K of step 2: MAPF_EINVAL on a null env or k outside 1..8, and nothing changes
 * then.  It has an effect only while the human weight is above 0.  No device call; in force from the
 * next mapf_pibt_actions / mapf_rollout_pibt launch; a captured launch keeps the horizon of its
 * capture.  Resets and mapf_set_state do not touch it. */
int mapf_set_pibt_human_horizon(mapf_env *env, int32_t k);
/* The handle's human horizon, or MAPF_EINVAL on a null env. */
int mapf_get_pibt_human_horizon(const mapf_env *env);
/* P_1..P_8 of step 2 for the current state of every env: cells DEVICE uint32 [B][8], packed as `pos`
 * is (row | col << 16), 0xFFFFFFFF (NO_CELL) past the path's end -- all eight, whatever the handle's
 * horizon, by the lookup the picks run: a wrong cell can be told from a wrong price.  MAPF_ESTATE
 * before mapf_reset. */
int mapf_pibt_human_cells(mapf_env *env, uint32_t *cells, void *stream);
/* The word the kernels take weight, radius, constr_d2 and horizon in, on the host (the functions
 * the kernels run): returns it (0 for weight 0) and, with fields != NULL, unpacks it into
 * fields[4] = weight, radius, constr_d2, horizon.  With k = 1 the word is
 * weight | radius << 8 | constr_d2 << 16.  -1 for weight outside 0..16, radius outside 1..64,
 * constr_d2 outside 0..4095 or k outside 1..8. */
int mapf_pibt_w_word(int32_t weight, int32_t penalty_radius, int32_t constr_d2, int32_t k, int32_t *fields);
/* level(penalty_radius, d2) of step 2, on the host (the function the kernels run).  MAPF_EINVAL
 * for a radius outside 1..64 or d2 < 0. */
int mapf_pibt_human_level(int32_t penalty_radius, int32_t d2);
/* Step 3 on the host, plain sequential code with no device call: pos [n][2] (row, col), key [n][5]
 * (negative = not admitted), age [n] -> actions [n]; bit i of *failed = agent i's pick failed.
 * MAPF_EINVAL on n outside 1..64, a null pointer or two agents on one cell. */
int mapf_pibt_host(int32_t n, const int32_t *pos, const int32_t *key, const uint32_t *age, int32_t *actions,
                   uint64_t *failed);
/* The PIBT policy, T steps: T x (mapf_pibt_actions, mapf_step_observe) -- identical results -- as
 * ONE launch where mapf_rollout_random_fused says so: the rollout kernels' PIBT forms pick in the
 * stepping wave from the tiled maps (pair-lane kernel: the solve over the agents' head lanes, the
 * picks handed over through the descent policy's LDS row), the age pair in registers across the
 * steps and written back at the end, so the handle's arrays are exactly as T per-step picks
 * leave them.  actions_out receives the chosen actions; slots (MAPF_SLOTS, MAPF_SLOTS_BAND_CLEAN,
 * MAPF_SLOTS_OBS_BITS) / actions_out / out / obs / vec, the capture rules and T = 0: as
 * mapf_rollout_descent.  Requires keep_bfs (MAPF_ESTATE otherwise). */
int mapf_rollout_pibt(mapf_env *env, int32_t T, int32_t slots, int32_t *actions_out, const mapf_step_out *out,
                      float *obs, float *vec, void *stream);
/* mapf_rollout_plan for mapf_rollout_pibt: the same text with ",pibt" inside the angle brackets,
 * e.g. "rollout_random_kernel<true,4,pibt>", "rollout_wide3_kernel<u64,1,true,pibt>" (the pair-lane
 * text ends as descent's, the wide three-wave form says bfsobs=0).  The text names the FORM: the
 * PIBT kernels take the age arrays as well, so the symbols a profiler shows are
 * rollout_random_pibt_kernel<ST,SUBS,BAND>, rollout_wide_pibt_kernel<T,RW,ST> and
 * rollout_wide3_pibt_kernel<T,RW,ST> with the same leading template arguments (ST: 0 plain stores,
 * 1 nontemporal -- printed "false" / "true" --, 2 packed bits).  Kind 0:
 * "pibt_actions+step_observe", the per-step launches.  With a human weight w > 0 the text ends
 * with " human_weight=<w>" -- a run-time argument of the same kernels --, followed by
 * " human_horizon=<K>" where K > 1; with w = 0 nothing is added. */
int mapf_rollout_pibt_plan(const mapf_env *env, int32_t slots, char *buf, int32_t n);

/* Action noise on the picked policies' rollouts (noise injection into a supervisor's trajectories, as in
 * DART, Laskey et al.): the policy's pick stays the LABEL, and with probability eps a uniform random
 * action is PLAYED in its place, so the trajectory drifts into states the planner alone never visits
 * while every label remains the planner's.  Per handle one integer noise_q16 in 0..65536, eps in
 * 1/65536 units, 0 by default.  It applies to the descent and the PIBT policy only (mapf_rollout_descent,
 * mapf_rollout_pibt, and mapf_rollout_sparse / mapf_rollout_perf under those policies); the random and
 * the tape policy ignore it: same results, same plan text.  For env b, agent i at clock t (steps since
 * reset, the clock the pick sees), label = the policy's pick:
 *   e      = philox(env_offset + b, P_NOISE | (i >> 3) << 8, t, 0; key = the handle's seed), P_NOISE = 12;
 *   u      = 16-bit half-word i & 7 of e: word (i & 7) >> 1, shifted right by ((i & 7) & 1) * 16 (the
 *            extraction of the random policy's action);
 *   noisy  = u < noise_q16: never at 0, always at 65536, with probability exactly noise_q16 / 65536;
 *   played = noisy ? the random policy's action for that agent and clock (what mapf_random_actions
 *            gives: draw P_ACT | (i >> 3) << 8) : label.
 * actions_out of the rollout calls receives `label`; the step is taken with `played`;
 * out->actions_fixed is, as always, what was executed after fixActions.  The PIBT ages are updated by
 * the pick as without noise (they depend on goals and clocks only).  With noise_q16 == 0 no draw is
 * made and every byte of every output and of the handle's state is as without the setting; with 65536
 * a descent or PIBT rollout equals the random policy's in everything but actions_out.  The draws are
 * counter-based on the env clock: any chunking of T, a captured launch replayed and T per-step calls
 * (pick, mapf_noise_actions, step) give the same bytes.
 *
 * mapf_set_action_noise: MAPF_EINVAL on a null env or a value outside 0..65536, and nothing changes
 * then.  No device call; the value is an argument of the next launch.  A captured launch keeps the value
 * it was captured with (its argument block is stored at capture).  Resets and mapf_set_state do not
 * touch it.  While the value is above 0 the descent and PIBT rollouts run instantiations of their own --
 * a launch without noise runs the kernels of a build without the feature, register for register -- and
 * their *_plan texts say so: ",noise" before the closing angle bracket, e.g.
 * "rollout_random_kernel<true,4,pibt,noise>", "rollout_wide_kernel<u64,1,descent,perf,noise>", and
 * " noise=<q16>" at the end, after the PIBT words (the per-step route: "pibt_actions+step_observe
 * noise=<q16>", the noise launch between the two).  At 0 nothing is added. */
int mapf_set_action_noise(mapf_env *env, int32_t noise_q16);
/* The handle's noise_q16, or MAPF_EINVAL on a null env. */
int mapf_get_action_noise(const mapf_env *env);
/* The rule for the current state (clock) of every env: labels DEVICE int32 [B][N] in, played DEVICE
 * int32 [B][N] out; played may be labels.  One small launch, capturable; at noise 0 it copies.  Labels
 * are not validated (a step refuses bad actions as ever).  MAPF_ESTATE before mapf_reset. */
int mapf_noise_actions(mapf_env *env, const int32_t *labels, int32_t *played, void *stream);
/* `played` of the rule on the host, no device call (the function the kernels run).  MAPF_EINVAL for an
 * agent outside 0..63, a label outside 0..4 or noise_q16 outside 0..65536. */
int mapf_action_noise_pick(uint64_t seed, uint32_t env_id, int32_t agent, uint32_t clock, int32_t noise_q16,
                           int32_t label);

/* Copy agent.bfsMap for every agent: DEVICE int16 [B][N][H][W] (requires keep_bfs). */
int mapf_bfs(mapf_env *env, int16_t *dist, void *stream);

/* renderWorld (util.py:189-232; MapfGym._render, mapf_gym.py:639-646) for n envs at once:
 * envs = DEVICE int32 [n] env indices, frames = DEVICE uint8 [n][H*scale][W*scale][3] RGB.
 * Cells white / black, the human's remaining path as grey arrows and a star, agents' cells
 * in hsv(i / N, 1, 1), their goals as discs, the human as a grey triangle, painted in the
 * reference's order.  Polygons cover the pixels inside or on them (the reference uses cv2,
 * absent here: its edge rasterisation may differ by a pixel).  scale in 4..64. */
int mapf_render(mapf_env *env, const int32_t *envs, int32_t n, int32_t scale, uint8_t *frames, void *stream);

/* Counters of impossible states / clamped events (host uint32[16]); synchronises the stream. */
int mapf_get_counters(mapf_env *env, uint32_t *host16, void *stream);

/* Phase-cycle sums over the waves of the last step launch, recorded by the
 * -DMAPF_STAMPS diagnostic build ([15] = waves; all zero in the product
 * build): host uint64[16]; synchronises. */
int mapf_get_profile(mapf_env *env, uint64_t *host16, int reset, void *stream);
/* Diagnostic builds only: the fused kernel's per-workgroup timeline of its last
 * launch, host [nblocks][8] u64 (100 MHz realtime stamps 0-3, HW_ID, XCC_ID). */
int mapf_get_timeline(mapf_env *env, uint64_t *host, int32_t nblocks, void *stream);
/* Diagnostic build: per-wave phase cycles of the last step launch, uint64 [nwaves][8]
 * (slots 0-6 phases, 7 = 1 if the wave recorded). */
int mapf_get_wave_profile(mapf_env *env, uint64_t *host, int32_t nwaves, void *stream);

int mapf_get_state(mapf_env *env, const mapf_state *host, void *stream);   /* synchronises */
int mapf_set_state(mapf_env *env, const mapf_state *host, void *stream);   /* synchronises */

/* GAE over a [T][M] buffer (runner.py:117-149, numpy float32 semantics:
 * f32(gamma) and f32(gamma*lam) constants, separate multiply and add).
 * All pointers DEVICE float; v_last [M]. */
int mapf_gae(const float *rewards, const float *values, const float *v_last, float *adv, float *ret,
             int32_t T, int32_t M, double gamma, double lam, void *stream);

/* model.py:106-113: adv = norm(ret - v); cadv = norm(cret - cv);
 * norm(x) = (x - mean) / (std_unbiased + 1e-6); if mix: adv = (adv - lam*cadv)/(lam+1).
 * DEVICE float [M] each; adv_out / cadv_out [M]. */
int mapf_normalize_advantages(const float *ret, const float *v, const float *cret, const float *cv,
                              float *adv_out, float *cadv_out, int32_t M, double lagrange, int32_t mix,
                              void *stream);

/* mapf_normalize_advantages with the multiplier in DEVICE memory, lam_dev[2] = {f32(lagrange),
 * f32(lagrange + 1)} (computed on the host in double, as mapf_normalize_advantages does): the
 * form a captured hipGraph of the update replays with a new multiplier every update. */
int mapf_normalize_advantages_dlam(const float *ret, const float *v, const float *cret, const float *cv,
                                   float *adv_out, float *cadv_out, int32_t M, const float *lam_dev, int32_t mix,
                                   void *stream);

/* mapf_normalize_advantages over a minibatch split across ranks (model.py:106-113 on the GLOBAL
 * minibatch).  Per rank, x = ret - v and c = cret - cv over its M rows, in fp64:
 *   mapf_advantage_moments(mean = NULL): out[2] = {sum x, sum c}                -> all-reduce (sum)
 *   mapf_advantage_moments(mean = {mean x, mean c}): out[2] = {sum (x - mean x)^2, sum (c - mean c)^2}
 *                                                                            -> all-reduce (sum)
 *   mapf_normalize_advantages_stats(stats = {mean x, mean c, var x, var c}, unbiased over all ranks'
 *                                   rows): the normalisation of mapf_normalize_advantages.
 * mean, out, stats: DEVICE double pointers; the other arrays DEVICE float [M]. */
int mapf_advantage_moments(const float *ret, const float *v, const float *cret, const float *cv, int32_t M,
                           const double *mean, double *out, void *stream);
int mapf_normalize_advantages_stats(const float *ret, const float *v, const float *cret, const float *cv,
                                    const double *stats, float *adv_out, float *cadv_out, int32_t M, double lagrange,
                                    int32_t mix, void *stream);
/* mapf_normalize_advantages_stats with the multiplier in DEVICE memory, lam_dev[2] as in
 * mapf_normalize_advantages_dlam: the distributed form of Model.train's device update (the
 * multiplier stays where the captured single-rank form keeps it). */
int mapf_normalize_advantages_stats_dlam(const float *ret, const float *v, const float *cret, const float *cv,
                                         const double *stats, float *adv_out, float *cadv_out, int32_t M,
                                         const float *lam_dev, int32_t mix, void *stream);

/* OneEpPerformance.episodeReward / episodeCostReward of every env (runner.py:95-96:
 * `perf.episodeReward += np.sum(rewards)` once per step): x DEVICE float [T][B][N] (one
 * rollout's rewards, goal reward included, or cost rewards); out DEVICE float [B] = the float32
 * sum over t, in order, of numpy's float32 np.sum of x[t][b][0..N-1] (pairwise order; N <= 128). */
int mapf_episode_sum(const float *x, int32_t T, int32_t B, int32_t N, float *out, void *stream);

/* OneEpPerformance of one env (util.py; runner.py:64-99, evaluate.py:237-265): the eight numbers a
 * planner comparison reads, in episodes.METRIC_KEYS' order.  The float sums are the reference's own
 * arithmetic: per step numpy's pairwise float32 np.sum over the env's N values (sequential below 8
 * values; else 8 strided accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder in
 * order, then 0 + res), then acc = acc + step in float32 -- no contraction, no reassociation. */
typedef struct mapf_perf {            /* 32 bytes                                                */
    float   episode_reward;           /* sum_t np.sum(reward_total[t][b][:])  float32, in order   */
    float   episode_cost_reward;      /* sum_t np.sum(cost[t][b][:])          float32, in order   */
    int32_t human_collide;            /* status == -2                                            */
    int32_t static_collide;           /* status == -1                                            */
    int32_t agent_collide;            /* status == -3                                            */
    int32_t total_goals;              /* goals_reached == 1                                      */
    int32_t shadow_goals;             /* sum of shadow_goals                                     */
    int32_t constraint_violations;    /* constraints == 1 (jointStep adds int(.. >= 0.01))        */
} mapf_perf;

/* Reduce step outputs that already exist: `out` holds DEVICE [T]-slot outputs (status, reward_total,
 * cost, goals_reached, constraints [T][B][N]; shadow_goals [T][B]; T = 1: one step's [B] buffers),
 * perf is DEVICE [B].  One launch; accumulate = 0 starts from zero, 1 continues from what perf holds
 * (the float sums go on in order, so any chunking of an episode gives the bits of one call).  A NULL
 * field of out leaves the metrics it feeds at their previous value (or zero).  Nothing is launched for
 * T = 0.  Capturable, allocates nothing, does not synchronise; needs no env handle (as mapf_gae). */
int mapf_perf_accumulate(const mapf_step_out *out, int32_t T, int32_t B, int32_t N, mapf_perf *perf,
                         int32_t accumulate, void *stream);
/* One step of one env added to *perf on the HOST by the same function the kernels run (HOST arrays of
 * N values; a NULL array or shadow_goals < 0 leaves its metrics).  No device call. */
int mapf_perf_add_host(mapf_perf *perf, int32_t N, const int8_t *status, const float *reward_total,
                       const float *cost, const float *goals_reached, int32_t shadow_goals,
                       const float *constraints);

/* T committed steps of `policy` (0 random, 1 tape, 2 descent, 3 pibt: mapf_rollout_sparse's) in one
 * launch that writes DEVICE perf [B] and nothing else per step: no observation, no vec, no step
 * output.  `actions`: the [T][B][N] tape (policy 1, required); under the other policies NULL (nothing
 * written) or [T][B][N] receiving the drawn / chosen actions.  Everything the handle holds ends exactly
 * as after mapf_rollout_<policy>(T, ...): a following mapf_observe, mapf_step, mapf_pibt_actions or
 * rollout gives the same bytes.  The PIBT human weight and horizon apply as in mapf_rollout_pibt.
 * accumulate as in mapf_perf_accumulate; T = 0 does nothing and leaves perf untouched.
 * Kinds (mapf_rollout_random_fused): 1 the pair-lane kernel's perf form, 2 the one-wave-per-env
 * kernel's (the stepping role alone), 0 T x (the policy's pick, mapf_step with MAPF_STEP_COMMIT into a
 * [B][N] step scratch the handle owns, mapf_perf_accumulate with T = 1; with NULL actions the picks of
 * a step pass through a [B][N] row of that scratch).  mapf_create allocates the scratch only on handles
 * the one-wave-per-env kernel does not cover; the call allocates nothing.
 * Errors, all before any launch: MAPF_ESTATE descent / pibt without keep_bfs; MAPF_EINVAL null perf,
 * bad policy, tape with null actions.  Capturable as the other rollouts. */
int mapf_rollout_perf(mapf_env *env, int32_t policy, int32_t T, int32_t *actions, mapf_perf *perf,
                      int32_t accumulate, void *stream);
/* The form as text, with ",perf" inside the angle brackets: "rollout_random_kernel<..,pibt,perf>",
 * "rollout_wide_kernel<u64,1,descent,perf>"; kind 0: "<pick>+step+perf_accumulate" (e.g.
 * "pibt_actions+step+perf_accumulate", random: "step+perf_accumulate").  PIBT weight / horizon
 * suffixes as mapf_rollout_pibt_plan.  Returns the kind. */
int mapf_rollout_perf_plan(const mapf_env *env, int32_t policy, char *buf, int32_t n);

/* Model.step sampling (model.py:38-40): per row, inverse CDF of ps[M][5]
 * with a Philox uniform (key seed, counter (row, step)).  DEVICE. */
int mapf_sample_actions(const float *ps, int32_t ps_stride, int32_t *actions, int64_t *actions64, int32_t M,
                        uint64_t seed, uint32_t step, void *stream);

/* ---- PPO epochs over a whole device rollout: minibatch rows and their gather (csrc/mapf_minibatch.hip) ----
 *
 * mapf_minibatch_rows: rows_out[j] = P(start + j) for j < count, DEVICE int64 [count], where P is a
 * bijection of [0, n) fixed by (seed, epoch, n).  Stateless: every output is computed on its own
 * (no sort, no scratch of size n, no host data), so a minibatch is any window [start, start + count)
 * of the epoch's permutation.  Specification (csrc/mapf_common.h: shuffle_index, the one
 * __host__ __device__ function both entry points run):
 *   h    = the smallest integer >= 1 with 2^(2h) >= n (h <= 32); mask = 2^h - 1
 *   k[0..7] = the two Philox4x32-10 draws with key `seed` and counter
 *             (low 32 bits of n, P_SHUFFLE | d << 8, epoch, high 32 bits of n), d = 0, 1 (P_SHUFFLE = 11),
 *             taken x, y, z, w of draw 0 then of draw 1; rounds use k[0..5]
 *   x -> E(x), a 6-round balanced Feistel network over 2h bits: (L, R) = (x >> h, x & mask), then per
 *             round i: (L, R) <- (R, L ^ (F(R + k[i]) & mask)) in uint32 arithmetic, with
 *             F(v): v ^= v >> 16; v *= 0x7FEB352D; v ^= v >> 15; v *= 0x846CA68B; v ^= v >> 16;
 *             E(x) = L << h | R
 *   P(i) = the first of E(i), E(E(i)), ... that is < n (cycle walking: fewer than 4 steps expected).
 * MAPF_EINVAL for n < 1, start < 0, count < 0, start + count > n or a null rows_out with count > 0;
 * count == 0 launches nothing.  Asynchronous on `stream`; capturable. */
int mapf_minibatch_rows(uint64_t seed, uint32_t epoch, int64_t n, int64_t start, int64_t count, int64_t *rows_out,
                        void *stream);
/* The same rows into a HOST array, computed by the same function on the host: no device call, so it
 * works on a machine without a GPU. */
int mapf_minibatch_rows_host(uint64_t seed, uint32_t epoch, int64_t n, int64_t start, int64_t count,
                             int64_t *rows_out);

/* One gathered array of mapf_gather_rows: row j of dst = row rows[j] (env-major) of src. */
typedef struct mapf_gather_array {
    const void *src;         /* DEVICE, t-major [T][B][row_bytes]                           */
    void *dst;               /* DEVICE, [M][row_bytes]                                      */
    int64_t row_bytes;       /* a positive multiple of 4                                    */
} mapf_gather_array;

#define MAPF_GATHER_MAX 16

typedef struct mapf_gather_spec {
    int32_t T, B;            /* the rollout: T steps of B envs                              */
    int64_t M;               /* rows gathered                                               */
    const int64_t *rows;     /* DEVICE [M]: env-major row ids in [0, B*T)                   */
    int32_t count;           /* arrays, 1..MAPF_GATHER_MAX                                  */
    int32_t reserved;
    mapf_gather_array arrays[MAPF_GATHER_MAX];
} mapf_gather_spec;

/* Gathers `count` arrays in ONE launch: for every array a and every j < M, the row_bytes bytes of
 * a.dst at j * row_bytes are the bytes of a.src at ((rows[j] % T) * B + rows[j] / T) * row_bytes --
 * env-major row r is env r / T, step r % T of the t-major rollout buffers (the rows of
 * runner.EnvMajorRows).  No other byte is written; duplicate row ids are legal.
 * Row ids are NOT range-checked on the device: a row outside [0, B*T) reads outside src (the Python
 * wrapper checks explicit host indices; mapf_minibatch_rows produces rows in range by construction).
 * An array whose src, dst and row_bytes are all multiples of 16 moves in 16-byte loads and stores; any
 * other array in 4-byte ones (src and dst 4-byte aligned), decided per array on the host.  Grid: per
 * gathered row, one workgroup of 256 lanes per 4 KiB piece of each array with rows longer than 1 KiB;
 * the shorter arrays ride with the row's first workgroup.
 * MAPF_EINVAL, before any launch, on a null spec / rows / src / dst, count outside 1..16, a row_bytes
 * that is not a positive multiple of 4, a src or dst not 4-byte aligned, T, B or M < 1, or more than
 * 2^31 - 1 workgroups.  No host synchronisation and no allocation: capturable. */
int mapf_gather_rows(const mapf_gather_spec *spec, void *stream);

/* ---- Grid symmetries: every training row is eight (csrc/mapf_sym.h, csrc/mapf_sym.hip) ----
 *
 * The observation is an F x F window centred on the agent (F odd) and every channel is spatially
 * equivariant, so a row of (observation, vec, action, per-action columns) transformed by one of the
 * square's eight symmetries is the row the env would have produced on the transformed world.
 * A symmetry is g in 0..7: bit 2 = mirror the columns first, bits 0..1 = that many counter-clockwise
 * quarter turns after it.  On an F x F plane x, in numpy:
 *     np.rot90(np.flip(x, -1) if g & 4 else x, k=g & 3, axes=(-2, -1))
 * Rows grow downwards; action 1 is (0,+1), 2 is (+1,0), 3 is (0,-1), 4 is (-1,0).  Per generator:
 *                               quarter turn                      mirror
 *   cell (r, c)                 (F-1-c, r)                        (r, F-1-c)
 *   displacement (dr, dc)       (-dc, dr)                         (dr, -dc)
 *   action                      0 -> 0, 1 -> 4, 2 -> 1,           1 <-> 3
 *                               3 -> 2, 4 -> 3
 *   vec (v0, v1, v2, v3)        (0.0f - v1, v0, v2, v3)           (v0, 0.0f - v1, v2, v3)
 *   columns x[5] (train_valid,  out[action'(a)] = x[a]            out[action'(a)] = x[a]
 *   ps)
 * Negation is 0.0f - x, so a zero component stays +0.0 as the env computes it: vec is bit-equal to the
 * transformed world's.  An action outside 0..4 is copied unchanged.  The functions of csrc/mapf_sym.h
 * are the rule; the kernels and the host entry points below all run them.
 *
 * Host entry points (no device call; they work on a machine without a GPU):
 *   mapf_sym_cell      where cell (r, c) of an F x F plane goes under g
 *   mapf_sym_action    the action (any other value is returned as it is)
 *   mapf_sym_vec_host  vec float [n][4] -> out [n][4]
 *   mapf_sym_cols_host columns float [n][5] -> out [n][5]
 *   mapf_sym_obs_host  obs float [n_agents][C][F][F] -> out, every plane transformed (out != obs)
 *   mapf_sym_compose   the g whose effect is g1's, then g2's
 *   mapf_sym_inverse   the g that undoes g
 * MAPF_EINVAL for g outside 0..7, F < 1, a cell outside the plane, a null pointer, n < 0. */
int mapf_sym_cell(int32_t g, int32_t F, int32_t r, int32_t c, int32_t *r2, int32_t *c2);
int64_t mapf_sym_action(int32_t g, int64_t a);
int mapf_sym_vec_host(const float *vec, int64_t n, int32_t g, float *out);
int mapf_sym_cols_host(const float *cols, int64_t n, int32_t g, float *out);
int mapf_sym_obs_host(const float *obs, int64_t n_agents, int32_t C, int32_t F, int32_t g, float *out);
int mapf_sym_compose(int32_t g1, int32_t g2);
int mapf_sym_inverse(int32_t g);

/* mapf_sym_draw: sym_out[j] for j < count, DEVICE uint8 [count], uniform over the set bits of the 8-bit
 * mask `allowed` (0xFF the whole group, 0x0F rotations only, 0x01 identity only).  Stateless, a pure
 * function of (seed, epoch, start + j): word = x of the Philox4x32-10 draw with key `seed` and counter
 * (low 32 bits of start + j, P_SYM, epoch, high 32 bits of start + j), P_SYM = 13; the pick is the
 * ((word * popcount(allowed)) >> 32)-th set bit of allowed, counted from bit 0.  MAPF_EINVAL for
 * allowed == 0 or > 0xFF, start < 0, count < 0, a null sym_out with count > 0; count == 0 launches
 * nothing.  Asynchronous on `stream`; capturable.  mapf_sym_draw_host: the same values into a HOST
 * array by the same function, no device call. */
int mapf_sym_draw(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed, uint8_t *sym_out,
                  void *stream);
int mapf_sym_draw_host(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed,
                       uint8_t *sym_out);

/* What mapf_gather_rows_sym does to one array's rows. */
#define MAPF_GATHER_PLAIN 0      /* bytes copied, as mapf_gather_rows                                   */
#define MAPF_GATHER_OBS_F32 1    /* float [N][C][F][F] -> the same shape, every plane transformed       */
#define MAPF_GATHER_OBS_BITS 2   /* uint32 [N][WPA] ("Packed observations") -> float [N][C][F][F]       */
#define MAPF_GATHER_VEC 3        /* float [N][4]                                                        */
#define MAPF_GATHER_ACTION32 4   /* int32 [N]                                                           */
#define MAPF_GATHER_ACTION64 5   /* int64 [N], src and dst 8-byte aligned                               */
#define MAPF_GATHER_COLS 6       /* float [N][5]: per-action columns (train_valid, ps)                  */

typedef struct mapf_gather_sym_array {
    const void *src;         /* DEVICE, t-major [T][B][src_row_bytes]                       */
    void *dst;               /* DEVICE, [M][dst_row_bytes]                                  */
    int64_t src_row_bytes;   /* positive multiples of 4; equal but for MAPF_GATHER_OBS_BITS */
    int64_t dst_row_bytes;
    int32_t kind;            /* MAPF_GATHER_*                                               */
    int32_t reserved;
} mapf_gather_sym_array;

typedef struct mapf_gather_sym_spec {
    int32_t T, B;            /* the rollout: T steps of B envs                              */
    int64_t M;               /* rows gathered                                               */
    const int64_t *rows;     /* DEVICE [M]: env-major row ids in [0, B*T)                   */
    const uint8_t *sym;      /* DEVICE [M]: g per gathered row (its low 3 bits); NULL = identity */
    int32_t N, C, F;         /* agents per row, channels, window                            */
    int32_t count;           /* arrays, 1..MAPF_GATHER_MAX                                  */
    mapf_gather_sym_array arrays[MAPF_GATHER_MAX];
} mapf_gather_sym_spec;

/* mapf_gather_rows with a symmetry per gathered row, in ONE launch: row j of every array's dst is row
 * rows[j] of its src (mapf_gather_rows' addressing: env-major row r is step r % T, env r / T)
 * transformed by sym[j] as the array's kind says.  A packed observation is unpacked and transformed in
 * the same pass -- no staging copy, no mapf_unpack_obs launch; with sym NULL (or g = 0) the result is
 * mapf_gather_rows' bytes (followed by mapf_unpack_obs' for MAPF_GATHER_OBS_BITS).  No byte outside
 * the destinations is written; duplicate rows are legal; rows are not range-checked.
 * Row lengths: OBS_F32 N*C*F*F*4 both sides; OBS_BITS N*WPA*4 -> N*C*F*F*4; VEC N*16; ACTION32 N*4;
 * ACTION64 N*8; COLS N*20; PLAIN any equal pair.
 * Grid: per gathered row, one workgroup of 256 lanes per 4 KiB piece of the DESTINATION row of each
 * array whose destination rows are longer than 1 KiB; the shorter arrays ride with the row's first
 * workgroup.  An observation whose dst and dst_row_bytes are multiples of 16 is stored in 16-byte
 * pieces, lane-contiguous, each lane finding its source cells through the inverse map; the packed words
 * under a piece are staged in LDS (5 KiB per workgroup).
 * MAPF_EINVAL, before any launch: what mapf_gather_rows refuses (null spec / rows / src / dst, count
 * outside 1..16, row lengths that are not positive multiples of 4, pointers not 4-byte aligned, T, B or
 * M < 1, more than 2^31 - 1 workgroups); a kind outside the list; N < 1; F outside 1..16 or C outside
 * 1..7; F even while sym != NULL (an even window is not centred on the agent: its transform is not an
 * observation the env can produce); a row length that does not match the kind and N, C, F; an int64
 * action array not 8-byte aligned.  mapf_last_error names the field.  No host synchronisation and no
 * allocation: capturable. */
int mapf_gather_rows_sym(const mapf_gather_sym_spec *spec, void *stream);

/* ---- Policy acting forward: fused elementwise epilogues (csrc/mapf_policy.hip) ----
 * SCRIMPNet.forward (net.py:101-155) under autocast with no grad (Model.step /
 * Model.value, model.py:26-69); each call replaces two or three of torch's passes
 * over one activation.  fp16 tensors are passed as uint16_t bit patterns; all
 * pointers DEVICE, contiguous; dropout p in [0, 1) (0 = off), masks from Philox(seed).
 *   nhwc_bias_relu       x[rows][C] = relu(x + bias)                 conv + F.relu (net.py:104-112)
 *   nhwc_bias_relu_pool2 out = maxpool2(relu(x + bias)), x [B][H][W][C] conv + relu + pool1/pool2
 *   layernorm_f16        y(fp16)[rows][512] = LayerNorm(x fp32, row stride)   transformer.py:7-24
 *   dropout_residual     x(fp32) += dropout(y fp16), n % 4 == 0        Residual(... do1/do2)
 *   gelu_dropout_f16     h = dropout(gelu(h)), n % 4 == 0               MLP_Block (transformer.py:27-45)
 *   tokens               x[B][L+1][D] = dropout(cat(cls, A*VV) + pos)  net.py:124-131 */
int mapf_nhwc_bias_relu(uint16_t *x, const uint16_t *bias, int64_t rows, int32_t C, void *stream);
int mapf_nhwc_bias_relu_pool2(const uint16_t *x, const uint16_t *bias, uint16_t *out, int32_t B, int32_t H, int32_t W,
                              int32_t C, void *stream);
int mapf_layernorm_f16(const float *x, int64_t x_row_stride, const float *gamma, const float *beta, uint16_t *y,
                       int64_t rows, int32_t dim, float eps, void *stream);
/* out[c] = fp16 of the fp32 sum over the rows of g fp16 [rows][C] (fixed order): a linear's bias
 * gradient (the training forward's 17-token linears, net._SplitKLinear; its short 2-D ones,
 * net._LinearBG).  C % 4 == 0, C <= 4096; work: 512 * C floats of scratch.  rows <= 8192 with C % 8 == 0
 * and g 16-B aligned: one launch (a block per 32 columns), else per-block partials then their sum.
 * rows == 0 zeroes out (g may then be NULL).  Capturable. */
int mapf_colsum_f16(const uint16_t *g, uint16_t *out, float *work, int64_t rows, int32_t C, void *stream);
/* Backward of p = maxpool2x2(relu(fp16(r + bias))) (mapf_nhwc_bias_relu_pool2's forward from the raw
 * conv output r fp16 NHWC [B][H][W][C]; the training forward's pooled conv layers, net.py:106-111):
 * dr gets dp at each window's first strictly greatest activation in (row, column) order -- torch's
 * max_pool2d argmax -- where that activation is > 0; 0 elsewhere, including rows / columns no window
 * covers.  dbias = fp16 of the fp32 sum of dr over B, H, W.  work: 512 * C floats.  Capturable. */
int mapf_relu_bias_pool_bwd_f16(const uint16_t *r, const uint16_t *bias, const uint16_t *dp, uint16_t *dr,
                                uint16_t *dbias, float *work, int32_t B, int32_t H, int32_t W, int32_t C,
                                void *stream);
/* Backward of y = relu(conv + bias) over NHWC fp16 rows [rows][C] (mapf_nhwc_bias_relu's forward; the
 * training forward's conv layers): dx = dy where y > 0 else 0 (fp16, [rows][C]), dbias = fp16 of the
 * fp32 sum of dx over the rows (fixed order).  C % 4 == 0, C <= 1024; work: 512 * C floats of
 * scratch.  rows == 0 zeroes dbias.  Capturable. */
int mapf_relu_bias_bwd_f16(const uint16_t *y, const uint16_t *dy, uint16_t *dx, uint16_t *dbias, float *work,
                           int64_t rows, int32_t C, void *stream);
/* Multi-tensor casts in ONE launch (the training forward's fp16 copies of the fp32 weights under
 * autocast, and their fp16 gradients back to fp32: one launch each way instead of one per tensor):
 * dst[i][k] = (fp16) src[i][k] (round to nearest even) or the exact reverse, k < n[i], i < count <= 64.
 * src / dst / n are HOST arrays of device pointers and element counts (copied into the launch's
 * arguments; capturable).  MAPF_EINVAL on a bad count or a null pointer with n[i] > 0. */
int mapf_cast_f32_to_f16_multi(const float *const *src, uint16_t *const *dst, const int64_t *n, int32_t count,
                               void *stream);
int mapf_cast_f16_to_f32_multi(const uint16_t *const *src, float *const *dst, const int64_t *n, int32_t count,
                               void *stream);
/* mapf_cast_f32_to_f16_multi where entry i with cout[i] > 0 is a conv weight stored [Cout][ks][ks][Cin]
 * (channels_last [Cout][Cin][ks][ks], Cout = cout[i], ks = ks[i], Cin = n[i] / (Cout ks ks)) written as
 * its flipped, transposed copy [Cin][ks][ks][Cout]: dst[ci][ky][kx][co] = src[co][ks-1-ky][ks-1-kx][ci]
 * -- the weight of the data gradient dx = conv(dy, w flipped, transposed) (_HipConv) -- in the same launch
 * as the plain casts (cout[i] == 0).  cout / ks: HOST int32 arrays.  MAPF_EINVAL as above or when n[i]
 * is not a multiple of Cout ks ks. */
int mapf_cast_f32_to_f16_multi_flip(const float *const *src, uint16_t *const *dst, const int64_t *n,
                                    const int32_t *cout, const int32_t *ks, int32_t count, void *stream);
/* Backward of z = fp16(LayerNorm(x)) (mapf_layernorm_f16; the training forward's PreNorm,
 * transformer.py:7-24 under autocast): given dz fp16 [rows][512], dx fp32 [rows][512] (contiguous),
 * dgamma / dbeta fp32 [512] (sums over the rows, fixed order).  mean / rstd are recomputed from x as
 * mapf_layernorm_f16 computes them.  dres: NULL, or fp32 [rows][512] added to dx -- the gradient the
 * residual path x + fn(LN(x)) brings to x, so the two need no separate add.  work: 2 * 512 * 512
 * floats of scratch.  rows == 0 zeroes dgamma / dbeta.  No host synchronisation, no memset:
 * capturable. */
int mapf_layernorm_bwd_f16(const float *x, int64_t x_row_stride, const float *gamma, const uint16_t *dz,
                           const float *dres, float *dx, float *dgamma, float *dbeta, float *work, int64_t rows,
                           int32_t dim, float eps, void *stream);

/* The TRAINING forward's dropout + residual + next LayerNorm (round 6; net._DropResLN), one pass:
 * x_out = res + dropout(y) (fp32; res rows res_row_stride floats apart, y fp16 contiguous), z =
 * fp16(LayerNorm(x_out)) -- mapf_dropout_residual_layernorm's arithmetic, out of place.  The dropout's
 * seed is read from DEVICE memory (seed_dev[0], a counter the training forward increments, mixed with
 * the site's salt), so a captured update draws new masks on every replay.  dim 512, p in [0, 1). */
int mapf_dropout_residual_layernorm_train(const float *res, int64_t res_row_stride, const uint16_t *y, float *x_out,
                                          const float *gamma, const float *beta, uint16_t *z, int64_t rows, int32_t dim,
                                          float eps, float p, const uint64_t *seed_dev, uint32_t salt, void *stream);
/* Its backward: mapf_layernorm_bwd_f16 over x_out (contiguous) with dres, plus dy (fp16) = the
 * gradient of the dropped branch: fp16(fp16(dx) * 1 / (1 - p)) where the forward kept, 0 elsewhere. */
int mapf_layernorm_dropout_bwd_f16(const float *x, const float *gamma, const uint16_t *dz, const float *dres, float *dx,
                                   uint16_t *dy, float *dgamma, float *dbeta, float *work, int64_t rows, int32_t dim,
                                   float eps, float p, const uint64_t *seed_dev, uint32_t salt, void *stream);
/* The training forward's MLP GELU + dropout (net._GeluDropout): out = dropout(gelu(h)) fp16 (h kept), and
 * its backward dh = fp16(gelu'(h) * fp16(dout / (1 - p)) where kept) -- torch's masked_scale then its exact
 * GeluBackward; the seed in device memory as above.  n % 4 == 0. */
int mapf_gelu_dropout_train_f16(const uint16_t *h, uint16_t *out, int64_t n, float p, const uint64_t *seed_dev,
                                uint32_t salt, void *stream);
int mapf_gelu_dropout_bwd_f16(const uint16_t *h, const uint16_t *dout, uint16_t *dh, int64_t n, float p,
                              const uint64_t *seed_dev, uint32_t salt, void *stream);
int mapf_dropout_residual(float *x, const uint16_t *y, int64_t n, float p, uint64_t seed, void *stream);
/* mapf_dropout_residual on rows x 512 contiguous x, y, then z = LayerNorm(x) as fp16 (like
 * mapf_layernorm_f16) in one pass; bit-identical to the two calls with the same seed. */
int mapf_dropout_residual_layernorm(float *x, const uint16_t *y, const float *gamma, const float *beta, uint16_t *z,
                                    int64_t rows, int32_t dim, float eps, float p, uint64_t seed, void *stream);
int mapf_gelu_dropout_f16(uint16_t *h, int64_t n, float p, uint64_t seed, void *stream);
int mapf_tokens(float *x, const float *A, const uint16_t *VV, const float *cls, const float *pos, int64_t B, int32_t L,
                int32_t D, float p, uint64_t seed, void *stream);
/* mapf_tokens (D = 512) and z = LayerNorm(x) as fp16 (gamma, beta, eps) in one pass; bit-identical
 * to mapf_tokens then mapf_layernorm_f16.  x may be NULL (the tokens not written: see
 * mapf_linear512_tokens_residual_layernorm). */
int mapf_tokens_layernorm(float *x, const float *A, const uint16_t *VV, const float *cls, const float *pos, int64_t B,
                          int32_t L, int32_t D, float p, uint64_t seed, const float *gamma, const float *beta,
                          float eps, uint16_t *z, void *stream);
/* The TRAINING forward's tokens and the first PreNorm (net._TokensLN; SCRIMPNet.forward, net.py:124-130):
 * x = dropout(cat(cls, A * VV) + pos) fp32 [B][L + 1][512] -- torch's ops and roundings (the product and
 * the sum rounded separately), dropout x * 1 / (1 - p) where kept, the mask from the device seed (graph-safe,
 * as mapf_dropout_residual_layernorm_train) -- and z = fp16(LayerNorm(x)) in one pass.  A: fp32 [B][L]
 * (the tokeniser's softmax), VV: fp16 [B][512], cls: fp32 [512], pos: fp32 [L + 1][512].  L == 16. */
int mapf_tokens_layernorm_train(float *x, const float *A, const uint16_t *VV, const float *cls, const float *pos,
                                int64_t B, int32_t L, float p, const uint64_t *seed_dev, uint32_t salt, const float *gamma,
                                const float *beta, float eps, uint16_t *z, void *stream);
/* Its backward after LayerNorm's (mapf_layernorm_bwd_f16 with the residual's gradient as dres): given
 * dx fp32 [B][L + 1][512], the same mask: g = dx / (1 - p) where kept; dA fp32 [B][L] = sum over the
 * columns of g[.][t + 1] VV; dVV fp16 [B][512] = sum over t of g[.][t + 1] A[.][t]; dpos fp32 [L + 1][512]
 * and dcls fp32 [512] the sums of g over B (fixed order).  work: 512 * (L + 1) * 512 floats. */
int mapf_tokens_train_bwd(const float *dx, const float *A, const uint16_t *VV, float *dA, uint16_t *dVV, float *dpos,
                          float *dcls, float *work, int64_t B, int32_t L, float p, const uint64_t *seed_dev,
                          uint32_t salt, void *stream);
/* Row tiles per workgroup of the mapf_linear512_* kernels (process-wide; bit-identical results
 * either way, for A/B timing): 2 (128 rows share each staged 512 x 32 weight chunk), 1 (64 rows),
 * or 0 (default: 1, the faster or within 1 % for every form at the c3 shape, round 5).  MAPF_EINVAL
 * on another value. */
int mapf_linear512_select(int32_t row_tiles);
/* LDS stages of the mapf_linear512_* kernels' K ring (process-wide, bit-identical results): 2, 3, 4
 * (stages - 1 weight/activation chunks in flight) or 0 (default, as measured).  MAPF_EINVAL otherwise. */
int mapf_linear512_stages(int32_t stages);
/* K per staged chunk of the mapf_linear512_* kernels (process-wide, bit-identical results: the same
 * MFMA sequence per element): 32 (64-B half-line LDS rows), 64 (full 128-B lines, two stages; with 2
 * row tiles all 160 KiB of a CU's LDS) or 0 (default: 32).  MAPF_EINVAL otherwise. */
int mapf_linear512_kdepth(int32_t k);

/* 512 x 512 Linear (w: fp16 [512 out][512 in], torch's layout; bias fp16 [512]) on `rows` contiguous fp16
 * rows a[rows][512] with its epilogue, one launch (MFMA GEMM; the linear's fp16 output stays on chip):
 *   mapf_linear512_gelu_dropout        out = dropout(gelu(a w^T + b)) fp16    = lin + mapf_gelu_dropout_f16
 *   mapf_linear512_residual_layernorm  x += dropout(a w^T + b); z = LayerNorm(x) fp16
 *                                                                  = lin + mapf_dropout_residual_layernorm
 * The same dropout masks as those kernels for the same seed (only the GEMM's summation order differs). */
int mapf_linear512_gelu_dropout(const uint16_t *a, const uint16_t *w, const uint16_t *bias, uint16_t *out, int64_t rows,
                                float p, uint64_t seed, void *stream);
int mapf_linear512_residual_layernorm(const uint16_t *a, const uint16_t *w, const uint16_t *bias, float *x,
                                      const float *gamma, const float *beta, uint16_t *z, int64_t rows, float eps,
                                      float p, uint64_t seed, void *stream);

/* mapf_linear512_residual_layernorm that writes the updated residual rows back only for rows
 * g % x_every == 0 (z for every row): before a block that keeps only token 0 of the stream
 * (the encoder's last block), the other tokens' fp32 rows are never needed again. */
int mapf_linear512_residual_layernorm_rows(const uint16_t *a, const uint16_t *w, const uint16_t *bias, float *x,
                                           const float *gamma, const float *beta, uint16_t *z, int64_t rows, float eps,
                                           float p, uint64_t seed, int32_t x_every, void *stream);

/* mapf_linear512_residual_layernorm on the first block's residual stream without it in HBM: the
 * input rows x (B sequences x (L + 1) tokens) are the tokens of mapf_tokens (A, VV, cls, pos,
 * tok_p, tok_seed: same values and mask bits) recomputed in the epilogue; x is written with
 * tokens + dropout(linear(a)), z = LayerNorm of it.  With mapf_tokens_layernorm(x = NULL, ...)
 * before it, the tokens' fp32 copy is never written nor read back. */
int mapf_linear512_tokens_residual_layernorm(const uint16_t *a, const uint16_t *w, const uint16_t *bias, float *x,
                                             const float *gamma, const float *beta, uint16_t *z, int64_t B, int32_t L,
                                             float eps, float p, uint64_t seed, const float *tok_A,
                                             const uint16_t *tok_VV, const float *tok_cls, const float *tok_pos,
                                             float tok_p, uint64_t tok_seed, void *stream);
/* out[B][q_rows][512] = softmax(q k^T * scale) v per head (heads = 16, head_dim = 32, n <= 32 tokens;
 * fp16 in/out, fp32 scores and softmax, P rounded to fp16 for P.V like flash SDPA) --
 * transformer.py:48-85's attention for the first q_rows queries.  Strides in fp16 elements between
 * consecutive tokens / sequences of q and of k, v (multiples of 8; q, k, v 16-B aligned). */
int mapf_attention_f16(const uint16_t *q, const uint16_t *k, const uint16_t *v, uint16_t *out, int64_t B, int32_t n,
                       int32_t q_rows, int64_t q_token_stride, int64_t q_seq_stride, int64_t kv_token_stride,
                       int64_t kv_seq_stride, int32_t heads, int32_t head_dim, float scale, void *stream);

/* The gradient of mapf_attention_f16 (the training forward's attention, transformer.py:48-85):
 * given q, k, v (strides as mapf_attention_f16), its fp16 output `out` and the output gradient
 * `dout` ([B][q_rows][heads * head_dim] at out_token_stride / out_seq_stride), writes dq (q's
 * strides) and dk, dv (k's / v's strides) as fp16: P recomputed in fp32, D = rowsum(dout * out).
 * n <= 32, heads 16, head_dim 32; every pointer 16-B aligned, strides multiples of 8. */
int mapf_attention_bwd_f16(const uint16_t *q, const uint16_t *k, const uint16_t *v, const uint16_t *out,
                           const uint16_t *dout, uint16_t *dq, uint16_t *dk, uint16_t *dv, int64_t B, int32_t n,
                           int32_t q_rows, int64_t q_token_stride, int64_t q_seq_stride, int64_t kv_token_stride,
                           int64_t kv_seq_stride, int64_t out_token_stride, int64_t out_seq_stride, int32_t heads,
                           int32_t head_dim, float scale, void *stream);
/* Which kernel mapf_attention_bwd_f16 launches (process-wide): 1 (default, round 6) the MFMA form, one
 * wave per (sequence, head), P and dS rounded to fp16 as MFMA operands; 0 the VALU form, one wave per
 * three heads, P and dS in fp32.  MAPF_EINVAL otherwise. */
int mapf_attention_bwd_select(int32_t form);

/* ---- PPO loss (model.py:115-175) ------------------------------------------
 * All loss terms of one minibatch update over R = rows x agents elements with A actions each,
 * plus d(all_loss)/d(new_ps, new_v, new_cv, policy_sig), in one launch.  Device pointers: fp32
 * new_ps / old_ps / policy_sig / train_valid [R][A], int64 action [R], fp32 new_v, old_v, returns,
 * new_cv, old_cv, cost_returns, advantage, cost_advantage [R]; sig_fp16 != 0 when policy_sig was
 * fp16 (autocast): its clamp bounds and 1 - sig round to fp16 like torch's.  HOST pointer coef[6]
 * = {CLIP_RANGE, ENTROPY_COEF, VALUE_COEF, VALID_COEF, COST_VALUE_COEF, COST_COEF * lambda}.
 * loss[1] (device) = all_loss; terms[7] (device) = {policy, entropy, critic, valid, cost critic,
 * cost, clip_frac}; the grads have the shapes of their inputs.  Deterministic (fixed-order reduction). */
int mapf_ppo_loss(const float *new_ps, const float *old_ps, const int64_t *action, const float *new_v,
                  const float *old_v, const float *returns, const float *new_cv, const float *old_cv,
                  const float *cost_returns, const float *advantage, const float *cost_advantage,
                  const float *policy_sig, int32_t sig_fp16, const float *train_valid, int64_t R, int32_t A,
                  const float *coef, float *loss, float *terms, float *grad_ps, float *grad_v, float *grad_cv,
                  float *grad_sig, void *stream);

/* SCRIMPNet's 128- and 256-channel convolutions (net.py:104-111: conv1a / conv1b 3x3 128->128,
 * conv2 2x2 128->256, conv2a / conv2b 2x2 256->256; and 2x2 256->128, conv2's data gradient over the
 * flipped weight in the training backward; stride 1, zero padding `pad`) as an MFMA
 * implicit GEMM (csrc/mapf_conv.hip).  x: fp16 NHWC [nimg][H][W][Cin]; w_packed: fp16
 * [Cout][ks][ks][Cin] (torch's weight permuted); y: fp16 NHWC [nimg][Ho][Wo][Cout], Ho = H + 2 pad -
 * ks + 1.  fp32 accumulation, output rounded to fp16; relu = 1: then + bias (fp16, rounded again)
 * and ReLU -- the autocast conv followed by mapf_nhwc_bias_relu.  MAPF_EINVAL for other shapes. */
int mapf_conv_nhwc_f16(const uint16_t *x, const uint16_t *w_packed, const uint16_t *bias, uint16_t *y, int64_t nimg,
                       int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t pad, int32_t relu,
                       void *stream);

/* mapf_conv_nhwc_f16 + bias + ReLU + 2x2 max-pool (net.py:106-107 / 110-111: relu(conv) then
 * MaxPool2d(2), floor), y fp16 NHWC [nimg][Ho / 2][Wo / 2][Cout]: the conv's output never goes to
 * HBM (tiles of whole images; 128 -> 128 3x3 and 256 -> 256 2x2 with Ho * Wo <= the tile).
 * Same values as mapf_conv_nhwc_f16(relu = 0) then mapf_nhwc_bias_relu_pool2. */
int mapf_conv_nhwc_pool_f16(const uint16_t *x, const uint16_t *w_packed, const uint16_t *bias, uint16_t *y, int64_t nimg,
                            int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t pad, void *stream);

/* Which implicit-GEMM form mapf_conv_nhwc_f16 / mapf_conv_nhwc_pool_f16 launch (process-wide; values
 * to fp16 rounding of a different summation order, for A/B timing): 2 the image-resident form
 * wherever its geometry applies (whole images per workgroup, each input channel slice DMA'd into
 * LDS once and read by every tap), 0 the per-tap staged form, 1 (default) the faster of the two
 * as measured per layer (image-resident for the 3x3 and the pooled layers).  MAPF_EINVAL on
 * another value. */
int mapf_conv_select(int32_t impl);

/* conv1 (net.py:104, 3x3, padding 1, Cin = num_channel <= 7, Cout = 128) from the fp32 NCHW observation
 * x_nchw [nimg][Cin][H][W] (cast to fp16 as autocast does); w fp16 [Cout][64]: torch's [Cout][Cin][3][3]
 * flattened per output channel (K = Cin * 9 in (c, ky, kx) order) and zero-padded to 64;
 * y fp16 NHWC [nimg][H][W][Cout] = relu(fp16(fp16(conv) + bias)) -- the MIOpen path's NHWC copy, cast,
 * conv and mapf_nhwc_bias_relu in one launch. */
int mapf_conv_first_f32(const float *x_nchw, const uint16_t *w, const uint16_t *bias, uint16_t *y, int64_t nimg,
                        int32_t Cin, int32_t H, int32_t W, int32_t Cout, void *stream);

/* ---- Packed observations: one bit per cell ----
 * Every observation value is 0.0 or 1.0.  With CFF = num_channel * fov * fov and WPA = ceil(CFF / 32),
 * an agent's packed observation is WPA little-endian uint32 words: bit k % 32 of word k / 32 is float
 * k of its [C][F][F] block (1 for 1.0f); the 32 * WPA - CFF padding bits of the last word are 0 and
 * always written.  Buffers are uint32 [..][N][WPA] wherever the float calls have float
 * [..][N][C][F][F] (c2: 92 B per agent against 2,904); `vec` is unchanged.  In numpy:
 * np.packbits(obs.reshape(A, CFF) != 0, axis=1, bitorder="little"), zero-padded to 4 * WPA bytes.
 *
 * mapf_obs_bits_words: WPA of a configuration (host only, no device call; <= 0 arguments give 0).
 * mapf_observe_bits / mapf_step_observe_bits: mapf_observe / mapf_step_observe writing
 * bits [B][N][WPA] on the device.  Where the float call would fork the pending search beside the
 * observe launch (wide maps, the BFS channel) and rewrite channel 6 as floats afterwards, the packed
 * call joins the search on the caller's stream before it observes, as mapf_tuning.serial_search = 1
 * does for the float call: there is no packed BFS fixup.
 * mapf_obs_pack_host / mapf_obs_unpack_host: the format on the host (obs [n_agents][C][F][F] floats,
 * non-zero packs as 1; bits [n_agents][WPA]), through the function the kernels run.
 * mapf_unpack_obs: bits [n_agents][WPA] on the device -> dst [n_agents][C][F][F] as 0 / 1 in fp32
 * (dst_f16 = 0) or fp16 (1); dst needs 4-byte alignment only.  Launches nothing for n_agents = 0;
 * capturable.
 * mapf_conv_first_bits: mapf_conv_first_f32 reading the packed observation (bits [nimg][WPA], one
 * image per agent, Cin = num_channel, H = W = fov); its output is bit-identical to
 * mapf_conv_first_f32 on the unpacked floats. */
int32_t mapf_obs_bits_words(const mapf_config *cfg);
int mapf_observe_bits(mapf_env *env, uint32_t *bits, float *vec, void *stream);
int mapf_step_observe_bits(mapf_env *env, const int32_t *actions, const mapf_step_out *out, uint32_t *bits, float *vec,
                           void *stream);
int mapf_obs_pack_host(const float *obs, int64_t n_agents, int32_t C, int32_t F, uint32_t *bits);
int mapf_obs_unpack_host(const uint32_t *bits, int64_t n_agents, int32_t C, int32_t F, float *obs);
int mapf_unpack_obs(const uint32_t *bits, void *dst, int64_t n_agents, int32_t C, int32_t F, int32_t dst_f16,
                    void *stream);
int mapf_conv_first_bits(const uint32_t *bits, const uint16_t *w, const uint16_t *bias, uint16_t *y, int64_t nimg,
                         int32_t Cin, int32_t H, int32_t W, int32_t Cout, void *stream);

/* mapf_ppo_loss with coef[6] in DEVICE memory (captured-graph updates: the Lagrangian term changes
 * every update without re-capturing). */
int mapf_ppo_loss_dcoef(const float *new_ps, const float *old_ps, const int64_t *action, const float *new_v,
                        const float *old_v, const float *returns, const float *new_cv, const float *old_cv,
                        const float *cost_returns, const float *advantage, const float *cost_advantage,
                        const float *policy_sig, int32_t sig_fp16, const float *train_valid, int64_t R, int32_t A,
                        const float *coef_dev, float *loss, float *terms, float *grad_ps, float *grad_v,
                        float *grad_cv, float *grad_sig, void *stream);

/* ---- Imitation loss (model.py:205-231: behaviour cloning) ------------------------------------
 * The cross-entropy of the policy logits against an expert's actions over R = rows x agents
 * elements with A actions each, plus its gradient, in one launch (csrc/mapf_imitation.hip).
 * Device pointers: logits [R][A] contiguous, fp32 (logits_f16 = 0) or fp16 bit patterns (1: the
 * autocast policy layer's output); action [R], int32 (action_i64 = 0: the rollout buffers) or
 * int64 (1: the reference's contract).
 *   loss[1]   = mean_r(logsumexp(l_r) - l_r[a_r]), rows in fp32 with their maximum subtracted:
 *               F.cross_entropy(logits.swapaxes(1, 2), optimal_action) of model.py:221-222.  With
 *               fp16 logits every log-probability is rounded to fp16 once (-inf past -65504), where
 *               torch's autocast cross_entropy rounds it, for the loss and for the gradient's softmax
 *   terms[2]  = {mean [argmax(l_r) == a_r] (the smallest index among the maxima),
 *                mean softmax(l_r)[a_r]}
 *   grad_logits[R][A] fp32 = (softmax(l_r)[k] - [k == a_r]) / R
 * An action outside 0..A-1 makes loss[0] NaN (no device assert).  Deterministic (fixed-order
 * reduction), no allocation, no host synchronisation: capturable.  MAPF_EINVAL before any launch
 * for a null pointer, R < 1, or A outside 2..16. */
int mapf_imitation_loss(const void *logits, int32_t logits_f16, const void *action, int32_t action_i64, int64_t R,
                        int32_t A, float *loss, float *terms, float *grad_logits, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPF_H */
