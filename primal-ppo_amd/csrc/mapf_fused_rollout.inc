// primal-ppo_amd/csrc/mapf_fused_rollout.inc -- the body of the pair-lane rollout kernels
// (mapf_fused.hip: rollout_random_kernel, rollout_random_pibt_kernel, rollout_sparse_kernel), included into each.  In scope:
// the template arguments ST, SUBS, BAND, the policy POL, the arguments e, T, ro and RO, the argument type of the policy's kernel (a dependent name
// in rollout_random_kernel, so that the PIBT branches' members are looked up only where they exist).
// PERF (rollout_perf_kernel, mapf_rollout_perf): the step, the policy's pick and the wave's own search work
// stay; nothing is observed and no step output is stored -- the values the stores would take are added to
// the wave's record (PerfAcc, mapf_perf.h), which is stored once after the loop.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int E = 4;                     // envs per workgroup, one per wave
    constexpr bool TAPE = rollout_pol(POL) == ROLLOUT_TAPE, DESCENT = rollout_pol(POL) == ROLLOUT_DESCENT, PIBT = rollout_pol(POL) == ROLLOUT_PIBT;
    // LEAN: the step loop's forms that save VALU issue (DESIGN.md 9s): the map rows copied to LDS once, the
    // stream zeroed in uint4s, phases 1-3 of the observation in the one-wave form, the slot's offset added in
    // the storing lanes.  Not PIBT's kernels, which stand at their register limit (122-128 VGPRs) and would
    // take scratch, and not the kernels with plain observation stores (in place), which measured slower with
    // them: both keep the code they had.
    constexpr bool LEAN = !PIBT && ST != OBS_PLAIN;
    constexpr bool NOISE = rollout_pol_noise(POL);      // DESCENT / PIBT with action noise: an instantiation of its own
    // XCD-aware env order: workgroups are dealt round-robin over the 8 XCDs, so workgroup w
    // takes env block (w % 8) * (grid / 8) + w / 8 -- each XCD owns one contiguous range of
    // envs, and the output lines that several envs share (status: 16 envs per 128-B line)
    // are completed in one XCD's L2 instead of leaving it as partial lines from several.
    const int nb = (int)gridDim.x;
    const int wg = (ro.xcd_remap && (nb & 7) == 0) ? ((int)blockIdx.x & 7) * (nb >> 3) + ((int)blockIdx.x >> 3)
                                                   : (int)blockIdx.x;
    const int sub = SUBS > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;   // this wave's quarter
    const int qt = (int)(threadIdx.x & 255);           // thread index within the quarter
    const int blk = wg * SUBS + sub;                   // the quarter's 4-env block
    const int b0 = blk * E;
    const int nenv = min(E, e.B - b0);
    const int le = qt >> 6;
    char *qsm = smem + (SUBS > 1 ? (size_t)sub * ro.sub_lds : 0);
    // [4 * SUBS] words: fair, each wave's steps done; paced, the ring of arrival counters (mapf_group.h)
    uint32_t *prog = reinterpret_cast<uint32_t *>(smem + (size_t)SUBS * ro.sub_lds);
    static_assert(SUBS == 1 || 4 * SUBS == PACE_RING, "the pacing ring takes the place of the per-wave counters");
    const int gw = sub * E + le;                       // the wave's index in the workgroup
    // PERF: no observation areas -- the four envs' map rows alone stand where the observation layout does
    // (rollout_perf_map_lds), then the same search scratch, path copies and picks' rows
    ObsLds L{};
    if constexpr (PERF) {
        L.rowsz = e.Hp * e.WW;
        L.mapc = reinterpret_cast<uint32_t *>(qsm);
    } else {
        L = obs_layout(e, E, qsm, true);
    }
    const size_t obs_sz = PERF ? rollout_perf_map_lds(e) : rollout_obs_lds(e);
    const size_t base_sz = PERF ? rollout_perf_lds_bytes(e, ROLLOUT_RANDOM) : rollout_lds_bytes(e, ROLLOUT_RANDOM);
    float4 *lut = reinterpret_cast<float4 *>(qsm + rollout_obs_lds(e) - 256);
    if (!PERF && qt < 16) lut[qt] = make_float4((float)(qt & 1), (float)((qt >> 1) & 1), (float)((qt >> 2) & 1), (float)(qt >> 3));
    // envs past B never count: fair, they start at the top; paced, they are not among the live waves
    if (SUBS > 1 && (int)threadIdx.x < 4 * SUBS)
        prog[threadIdx.x] = ro.fair <= 0 || wg * SUBS * E + (int)threadIdx.x < e.B ? 0u : 0xFFFFFFFFu;
    __syncthreads();
    if constexpr (!PERF) L.lut = lut;
    const size_t swl = srch::wave_lds<uint32_t, 1>(e.H, e.W);
    char *slds = qsm + obs_sz + (size_t)le * swl;
    uint32_t *lpath = reinterpret_cast<uint32_t *>(qsm + obs_sz + 4 * swl) + (size_t)le * e.Lmax;
    // TAPE: this wave's TAPE_K staged rows, after the quarter's path copies; DESCENT: its one row of picks
    int32_t *trow = nullptr;
    if constexpr (TAPE) trow = reinterpret_cast<int32_t *>(qsm + base_sz) + (size_t)le * TAPE_K * 8;
    if constexpr (DESCENT || PIBT) trow = reinterpret_cast<int32_t *>(qsm + base_sz) + (size_t)le * 8;
    const uint32_t mreg = obs_map_word(e, b0, nenv, (int)(threadIdx.x & 63));
    EnvRegs rs{};
    if (le < nenv) env_regs_load<8>(e, b0 + le, rs, lpath);
    uint32_t pseen = 0, psince = 0;          // PIBT: the age pair of agent lane >> 3 (used on its head lane)
    if constexpr (PIBT) {
        if (le < nenv) {
            const size_t ag = (size_t)(b0 + le) * e.N + (size_t)min((int)(threadIdx.x & 63) >> 3, e.N - 1);
            pseen = static_cast<const RO &>(ro).pibt_seen[ag];
            psince = static_cast<const RO &>(ro).pibt_since[ag];
        }
    }
    [[maybe_unused]] PerfAcc pacc;          // PERF: the record to continue from, among the prologue's loads
    if constexpr (PERF) {
        if (le < nenv) pacc = perf_acc_load(ro_perf(ro) + (b0 + __builtin_amdgcn_readfirstlane(le)), ro_accumulate(ro));
    }
    // every prologue load has landed before the loop: otherwise the compiler keeps a
    // register's load "pending" at the loop header and waits vmcnt(0) -- i.e. behind
    // all of the previous step's stores -- where the loop uses it
    if constexpr (PERF) __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0): the record's loads are scalar
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0), expcnt/lgkmcnt untouched
    // the lane's skip set, one bit per store of its env's slice, from the slice's address.  It is
    // the same at every step where the unit divides the slot stride (every slot of the env keeps
    // slot 0's alignment: c2); where it does not (B * env bytes not a multiple of the unit, e.g.
    // B = 37) the set moves with t and the loop computes it again for each slot.
    uint32_t band_mask = 0;
    bool band_moves = false;
    if constexpr (BAND == OBS_BAND) {
        band_moves = ((size_t)e.B * e.N * e.C * e.F * e.F * 4) % MAPF_BAND_UNIT != 0;
        if (le < nenv && !band_moves)
            band_mask = obs_band_skip_mask(e, MAPF_BAND_UNIT, (size_t)(ro.obs + (size_t)(b0 + le) * e.N * e.C * e.F * e.F),
                                           (int)(threadIdx.x & 63));
    }
    // the env's map rows in LDS, once: the map does not change within a launch, the observation and the
    // wave's searches read them at every step.  Lane k holds word k: rowsz <= 64 (regmap_fits, which
    // rollout_fusable requires)
    if constexpr (PERF || LEAN) {
        if (le < nenv) obs_wave_map(L, le, mreg);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    RSTAMP_BEGIN();
    // (a scalar condition: pace_wait's s_sleep ignores EXEC)
    const bool pacing = SUBS > 1 && ro.slack >= 0 && __builtin_amdgcn_readfirstlane(le) < nenv;
    const bool fair = SUBS > 1 && ro.fair > 0 && le < nenv;
    const int live = min(max(e.B - wg * SUBS * E, 0), 4 * SUBS);     // the workgroup's waves that own an env
    for (int t = 0; t < T; ++t) {
        const DevEnv &E = e;
        const RO &R = ro;
        if (pacing) {
            RSTAMP_WAIT0();
            pace_wait(prog, t, R.slack, live);
            RSTAMP_WAIT1();
        }
        if (fair) {
            if ((uint32_t)t > group_min(prog, 4 * SUBS) + (uint32_t)R.fair) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(2);
        }
        const size_t BN = (size_t)E.B * E.N;
        const size_t s = R.slots ? (size_t)t : 0;
        // SPARSE: the env-slot's 16 mask words.  Steps below `valid` read them here, at the top of the
        // step, by scalar loads (obs_sparse_old), and obs_emit stores the pieces that were or become
        // non-zero; later steps store every piece.  The address is uniform: the wave's env, the step.
        [[maybe_unused]] uint32_t *sp_words = nullptr;
        if constexpr (BAND == OBS_SPARSE) {
            const int lew = __builtin_amdgcn_readfirstlane(le);
            sp_words = ro_shadow(ro) + (s * (size_t)E.B + (size_t)(b0 + lew)) * OBS_SPARSE_WORDS;
            band_mask = 0xFFFFFFFFu;
            if (t < ro_valid(ro) && lew < nenv) band_mask = obs_sparse_old(sp_words, (int)(threadIdx.x & 63));
        }
        if constexpr (TAPE) {
            if ((t & (TAPE_K - 1)) == 0) {
                if (le < nenv) {        // rows [t, t + TAPE_K) of this env, inside [T][B][N]
                    // lane -> agent lane & 7 of rows (lane >> 3) + 8k; the opaque copy keeps the
                    // addresses out of the loop's invariants (hoisted, they held 20 VGPRs through
                    // the whole loop: 128 VGPRs and scratch in the band form)
                    int lane = (int)(threadIdx.x & 63);
                    asm volatile("" : "+v"(lane));
                    const int i = lane & 7, r0 = lane >> 3, nrow = min(TAPE_K, T - t);
                    const int32_t *src = R.actions + ((size_t)(t + r0) * E.B + (size_t)(b0 + le)) * E.N + i;
                    int32_t v[TAPE_K / 8];
#pragma unroll
                    for (int k = 0; k < TAPE_K / 8; ++k)
                        v[k] = (i < E.N && r0 + 8 * k < nrow) ? src[(size_t)(8 * k) * BN] : 0;
#pragma unroll
                    for (int k = 0; k < TAPE_K / 8; ++k) as_lds(trow)[lane + 64 * k] = v[k];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        if constexpr (DESCENT) {
            // The maps read here were written before the launch (visible by the launch boundary)
            // or by this very wave, in step_pairs_search_inline of an earlier step: one wave's
            // vector stores and loads, same CU, performed in program order -- wavefront scope, so
            // the fence emits nothing and only keeps the compiler from moving these int16 loads
            // over the search's uint4 stores; the loads' own vmcnt wait is the only wait.
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (le < nenv) {
                int lane = (int)(threadIdx.x & 63);
                asm volatile("" : "+v"(lane));          // addresses stay out of the loop's invariants (as the tape's)
                const int i = lane >> 3;
                const bool head = (lane & 7) == 0 && i < E.N;
                int a = 0;
                if (head) {
                    const size_t ai = (size_t)(b0 + le) * E.N + i;
                    a = descent_action(E, E.bfs + ai * bfs_cells(E.H, E.W), rs.pi, rs.clock, i);
                    if (!PERF || R.actions) R.actions[s * BN + ai] = a;      // PERF: no actions asked for, none stored
                }
                // action noise: the label is stored, the step reads `played` from the row (N <= 8: one draw
                // group, env and clock the wave's)
                if constexpr (NOISE)
                    a = noise_play_wave(E.seed, E.env_offset + (uint32_t)(b0 + le), rs.clock, E.noise_q16, E.N, head, i, a);
                if (head) as_lds(trow)[i] = a;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if constexpr (PIBT) {
            // the maps: descent's visibility rule above (this wave searched what it reads)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (le < nenv) {
                int lane = (int)(threadIdx.x & 63);
                asm volatile("" : "+v"(lane));          // addresses stay out of the loop's invariants (as the tape's)
                const int i = lane >> 3;
                const bool head = (lane & 7) == 0 && i < E.N;
                const size_t ai = (size_t)(b0 + le) * E.N + (size_t)min(i, E.N - 1);
                uint32_t cand[NA] = {PIBT_NONE, PIBT_NONE, PIBT_NONE, PIBT_NONE, PIBT_NONE};
                uint32_t age = 0;
                if (head) {
                    age = pibt_age(pseen, psince, rs.gi, rs.clock);
                    const unsigned sm = E.smask[(E.shared_map ? 0 : (size_t)(b0 + le) * E.H * E.W) + prow(rs.pi) * E.W + pcol(rs.pi)];
                    // the human's predicted cells past hn: uniform-address reads of the wave's LDS copy of
                    // its current path (re-copied at a switch), made scalars for the loop's branch
                    pibt_candidates(E, E.bfs + ai * bfs_cells(E.H, E.W), rs.pi, sm, rs.hp, rs.hn, rs.clock, i, cand, [&](int j) {
                        return (uint32_t)__builtin_amdgcn_readfirstlane(
                            (int)human_ahead(as_lds(rs.lp), rs.hs, rs.hcur ? rs.hlen1 : rs.hlen0, j));
                    });
                }
                int a = pibt_solve_wave<8>(E.N, lane, head ? rs.pi : NO_CELL, cand, age);
                if (head && (!PERF || R.actions)) R.actions[s * BN + ai] = a;
                if constexpr (NOISE)         // as descent's
                    a = noise_play_wave(E.seed, E.env_offset + (uint32_t)(b0 + le), rs.clock, E.noise_q16, E.N, head, i, a);
                if (head) as_lds(trow)[i] = a;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        // LEAN: the slot's offset goes into the head lanes' store indices (step_pairs_env's `so`, `sb`), not
        // into nine bumped 64-bit pointers per step
        StepOut o = PERF ? StepOut{} : R.out;
        if constexpr (!LEAN) {
            if (o.status) o.status += s * BN;
            if (o.reward) o.reward += s * BN;
            if (o.shadow_goals) o.shadow_goals += s * E.B;
            if (o.cost) o.cost += s * BN;
            if (o.train_valid) o.train_valid += s * BN * NA;
            if (o.actions_fixed) o.actions_fixed += s * BN;
            if (o.goals_reached) o.goals_reached += s * BN;
            if (o.constraints) o.constraints += s * BN;
            if (o.reward_total) o.reward_total += s * BN;
        }
        PairsDeferred dfr;
        [[maybe_unused]] StepVals pv;
        step_pairs_env<8, !PERF, true, true, TAPE || DESCENT || PIBT, PERF>(
            E, TAPE ? trow + (size_t)(t & (TAPE_K - 1)) * 8 : (DESCENT || PIBT ? trow : (PERF && !R.actions ? nullptr : R.actions + s * BN)), o,
            TAPE || DESCENT || PIBT ? 1u : 3u, 0,
            blk * 256 + qt, L, b0, RegMap{mreg, true}, dfr, &rs, PERF ? &pv : nullptr, LEAN ? s * BN : 0, LEAN ? s * (size_t)E.B : 0);
        if constexpr (PERF) {
            if (le < nenv) {
                perf_acc_step<8>(pacc, pv, E.N, (int)(threadIdx.x & 63));
                step_pairs_search_inline(E, dfr, slds, L.mapc + (size_t)le * L.rowsz, rs);
            }
        } else
        if (le < nenv) {
            const ObsGroup g = obs_wave_init(E, L, le, mreg, !LEAN, LEAN);
            if (BAND == OBS_BAND && band_moves)
                band_mask = obs_band_skip_mask(E, MAPF_BAND_UNIT,
                                               (size_t)(R.obs + (s * BN + (size_t)(b0 + le) * E.N) * E.C * E.F * E.F),
                                               (int)(threadIdx.x & 63));
            // a slot of the packed buffer is B * N * WPA words, not B * N * CFF floats
            float *ob;
            if constexpr (ST == OBS_BITS) ob = R.obs + s * BN * (size_t)obs_bits_words(E.C, E.F);
            else ob = R.obs + s * BN * E.C * E.F * E.F;
            // the store loop in groups of four (obs_store_wave_nt); PIBT's kernels stand at their register
            // limit and spill with it: they keep the loop of one store per trip
            // LEAN: phases 1-3 in the one-wave form (obs_wave_rows: N <= 8 by rollout_fusable's G == 8)
            obs_emit<false, ST, BAND, PIBT ? 0 : OBS_NT_GROUP, LEAN>(E, L, ob, R.vec + s * BN * 4, g, b0, false, band_mask);
            // SPARSE: what the slot holds now, for the next launch over it (the stream is whole until the
            // next step's obs_wave_init); ordinary vector stores of lanes 0, 4, .., 60
            if constexpr (BAND == OBS_SPARSE) obs_sparse_store(g.stream, L.swe, sp_words, (int)(threadIdx.x & 63));
            step_pairs_search_inline(E, dfr, slds, L.mapc + (size_t)le * L.rowsz, rs);
            if (pacing) pace_arrive(prog, t);
            else if (fair) publish_count(prog + gw, (uint32_t)(t + 1));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (le < nenv) env_regs_store<8>(e, b0 + le, rs);
    if constexpr (PIBT) {
        const int lane = (int)(threadIdx.x & 63);
        if (le < nenv && (lane & 7) == 0 && (lane >> 3) < e.N) {
            static_cast<const RO &>(ro).pibt_seen[(size_t)(b0 + le) * e.N + (lane >> 3)] = pseen;
            static_cast<const RO &>(ro).pibt_since[(size_t)(b0 + le) * e.N + (lane >> 3)] = psince;
        }
    }
    if constexpr (PERF) {
        if (le < nenv) perf_acc_store(pacc, ro_perf(ro) + (b0 + le), (int)(threadIdx.x & 63));
    }
    if (le < nenv) RSTAMP_END(b0 + le);
