"""GPU parity of the env kernels off their default penalty radius, prediction depth, costs and lifelong flag.

Every other GPU test builds its config with k_predict = 5, penalty_radius = 5, lifelong = 1 and the costs
-0.3 / -2 / -2 / -0.35 / +1.5 (collision_cost == human_collision_cost).  mapf_create takes penalty_radius
1..64, k_predict 0..64, either lifelong and any costs, and every kernel family has code that depends on
them: the reward selects and reward_total, the radial cost (a table in lanes while R*R < 64 in the pair-lane
kernels, fp64 sqrt from R = 8 on; an LDS copy in the one-wave-per-env kernel while it is at most 1 KiB),
the danger disc of channel 4 (per-row half-widths, the plus of R = 1, the whole window at R = 64), the
predicted cells of channel 5 (LDS rows of k_predict words; one lane per cell in the one-wave-per-env
kernel, which therefore stops at 63) and `reached`, which is never true with lifelong off.

PARAMS x SHAPES below run through test_gpu_parity.run_random_case (random policy; every output, observation
bit, vector and the state at the launch ends bit for bit against the C oracle, which honours all of these
fields) and, for `costs` and `nolife`, through rollout_harness under the descent policy (the random policy
reaches too few goals).  One dict of overrides configures the device and the oracle.  Every case asserts
the kernel that ran, and -- from oracle runs alone, oracle_counts / descent_run -- that its inputs hold the
events it is there for; the measured counts are in the tables of the tests' docstrings.
"""
import functools

import numpy as np
import pytest
import torch

import rollout_harness as H
from descent_ref import descent_actions
from oracle import oracle as O
from test_gpu_parity import build_maps, run_random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


# every cost exact in float32, all five distinct (the defaults have collision == human_collision)
PARAMS = {
    "costs": dict(action_cost=-0.25, collision_cost=-1.5, human_collision_cost=-3.0, repeat_cost=-0.5, goal_reward=2.25),
    "r1_k0": dict(penalty_radius=1, k_predict=0),        # the plus; no predicted cell (shp and shpn coincide)
    "r7_k1": dict(penalty_radius=7, k_predict=1),        # the last radius with the cost table in lanes
    "r8_k8": dict(penalty_radius=8, k_predict=8),        # the first on the fp64 sqrt path
    "r64_k63": dict(penalty_radius=64, k_predict=63),    # the largest; the last K the one-wave-per-env kernel takes
    "r2_k64": dict(penalty_radius=2, k_predict=64),      # the largest K
    "nolife": dict(lifelong=0),
}
# da = 1, hp = 1, 6 channels, 60 steps: the smallest shapes that still select each kernel family
SHAPES = {
    "pair": dict(B=18, H=16, W=16, n=6, fov=9, nch=6, steps=60, map="wh", da=1, hp=1),     # ragged against 4 envs per workgroup
    "wide": dict(B=8, H=12, W=12, n=16, fov=9, nch=6, steps=60, map="wh", da=1, hp=1),
    "small": dict(B=24, H=16, W=16, n=2, fov=9, nch=6, steps=60, map="wh", da=1, hp=1),
    # per-env random maps, not square, the BFS channel: the disc clipped at map edges
    "edge": dict(B=5, H=40, W=30, n=12, fov=7, nch=7, steps=46, map="rand", da=1, hp=1),
}
SEED = 0x5EED0000          # run_random_case's seed base: seed = SEED + len(name)
DESCENT_SEED = 0xE7A90000
LAUNCHES = (1, 23, 36)     # descent cases: steps per launch, 60 in all

RUNS = []                  # (shape, params, path, packed)
for _p in PARAMS:
    RUNS += [("pair", _p, "rollout", False), ("wide", _p, "rollout", False), ("small", _p, "plain", False),
             ("small", _p, "fused", False)]
RUNS += [("pair", _p, "inplace", False) for _p in ("r8_k8", "r64_k63")]
RUNS += [(_s, _p, "rollout", True) for _p in ("r7_k1", "r2_k64") for _s in ("pair", "wide")]
RUNS += [("edge", _p, "rollout", False) for _p in ("r1_k0", "r64_k63")]


def case_name(shape, params):
    """The name run_random_case derives the seed from: the same for every path of a (shape, params)."""
    return f"{shape}-{params}"


# ------------------------------------------------------------------ what the inputs hold, from the oracle alone
@functools.lru_cache(maxsize=None)
def oracle_counts(shape, name_len, params):
    """The events of run_random_case's episode for (shape, seed SEED + name_len, PARAMS[params] or the
    defaults for None), counted on the oracle alone: statuses, goals reached, agent-steps with
    cost > 0, bits of channels 4 and 5 over every step's observation, and (agent, step) pairs with
    the agent on its goal after the step."""
    case = SHAPES[shape]
    maps, shared = build_maps(case, case["B"], np.random.default_rng(5))
    cfg = O.make_config(case["H"], case["W"], case["n"], case["fov"], case["nch"], use_da=1, use_hp=1, human_mode=1,
                        goal_mode=1, fix_choice=1, seed=SEED + name_len, env_offset=7, **(PARAMS[params] if params else {}))
    c = dict(status={-1: 0, -2: 0, -3: 0, -4: 0, 1: 0}, goals=0, cost_pos=0, ch4=0, ch5=0, on_goal=0, errors=0)
    for b in range(case["B"]):
        oe = O.OracleEnv(cfg, env_id=7 + b)
        oe.reset_random(maps if shared else maps[b])
        for _ in range(case["steps"]):
            o = oe.step(oe.random_actions())
            for s in o["status"]:
                c["status"][int(s)] += 1
            c["goals"] += int(o["goals"].sum())
            c["cost_pos"] += int((o["cost"] > 0).sum())
            obs, _ = oe.observe()
            c["ch4"] += int(obs[:, 4].sum())
            c["ch5"] += int(obs[:, 5].sum())
            p, g = oe.agents()
            c["on_goal"] += int((p == g).all(1).sum())
        c["errors"] += oe.errors()
    return c


def assert_inputs(shape, params):
    """The conditions on a random-policy case's inputs (module docstring); prints the counts."""
    n = len(case_name(shape, params))
    c, base = oracle_counts(shape, n, params), oracle_counts(shape, n, None)
    print(f"{case_name(shape, params)}: {c}; at the defaults: cost>0 {base['cost_pos']} ch4 {base['ch4']} ch5 {base['ch5']}")
    assert c["errors"] == 0
    over = PARAMS[params]
    if params == "costs":
        for s in (-1, -2, -3, -4):
            assert c["status"][s] >= 5, (shape, s, c["status"])
    if "penalty_radius" in over:
        assert c["status"] == base["status"]               # the radius moves no agent
        assert c["cost_pos"] != base["cost_pos"] and c["ch4"] != base["ch4"], (shape, params, c, base)
        bigger = over["penalty_radius"] > 5
        assert (c["cost_pos"] > base["cost_pos"]) == bigger and (c["ch4"] > base["ch4"]) == bigger
    if "k_predict" in over:
        k = over["k_predict"]
        assert (c["ch5"] == 0) == (k == 0), (shape, params, c["ch5"])
        assert (c["ch5"] > base["ch5"]) == (k > 5) and (c["ch5"] < base["ch5"]) == (k < 5)
    if params == "nolife":
        assert c["goals"] == 0 and c["on_goal"] >= 20, (shape, c)
    return c


def test_predicted_cells_grow_with_k():
    """Channel 5 over the `pair` episode holds more bits at K = 8 than at K = 1, and at K = 63 than at 8."""
    bits = [oracle_counts("pair", len(case_name("pair", p)), p)["ch5"] for p in ("r1_k0", "r7_k1", "r8_k8", "r64_k63")]
    print("ch5 bits on pair at K = 0 / 1 / 8 / 63:", bits)
    assert bits[0] == 0 < bits[1] < bits[2] < bits[3]


# ------------------------------------------------------------------ the random policy
def expectations(shape, params, path, packed):
    """What the handle must report, so that a silent fall-back never counts as coverage."""
    tag = ",bits" if packed else ""
    if shape == "pair":                                     # five workgroups: never grouped
        return dict(expect_rollout_kernel=1, expect_name="rollout_random_kernel<%s,1%s>" % (
            "true" if path == "rollout" else "false", tag))
    if shape == "small":                                    # per-step launches; "fused": step + observe in one
        return dict(expect_fused=True) if path == "fused" else {}
    if shape == "wide" and params == "r2_k64":
        # 16 agents, the HP channel and 64 predicted cells: the one-wave-per-env kernel's snapshot holds one
        # cell per lane 1..63 and the pair-lane kernel stops at 8 agents -- no one-launch form, per-step launches
        return dict(expect_rollout_kernel=0, expect_name="step_observe" + ("_bits" if packed else ""))
    return dict(expect_rollout_kernel=2)                    # wide, edge: one wave per env


@pytest.mark.parametrize("shape,params,path,packed", RUNS, ids=["-".join([s, p, q] + ["bits"] * k) for s, p, q, k in RUNS])
def test_params_match_oracle(shape, params, path, packed):
    """Measured on the oracle (oracle_counts; 60 steps, `edge` 46; the seed follows the case's name, so the
    episodes of a shape differ between parameter sets).  In brackets: the same episode at the defaults
    (R = 5, K = 5).  `on goal`: (agent, step) pairs with the agent on its goal after the step.

        case            -1/-2/-3/-4       goals  cost > 0      ch4 bits          ch5 bits        on goal
        pair-costs      745/24/101/1270   12     1013          78178             4298            0
        wide-costs      1276/56/655/1403  25     2189          151845            7881            0
        small-costs     363/7/12/559      5      512           38653             1975            0
        pair-r1_k0      745/24/101/1270   12     16 (1013)     5722 (78178)      0 (4298)        0
        wide-r1_k0      1276/56/655/1403  25     37 (2189)     11888 (151845)    0 (7881)        0
        small-r1_k0     363/7/12/559      5      3 (512)       2784 (38653)      0 (1975)        0
        pair-r7_k1      745/24/101/1270   12     1950 (1013)   131782 (78178)    797 (4298)      0
        wide-r7_k1      1276/56/655/1403  25     3813 (2189)   237087 (151845)   1174 (7881)     0
        small-r7_k1     363/7/12/559      5      893 (512)     63927 (38653)     355 (1975)      0
        pair-r8_k8      745/24/101/1270   12     2483 (1013)   165648 (78178)    7705 (4298)     0
        wide-r8_k8      1276/56/655/1403  25     4673 (2189)   281706 (151845)   16165 (7881)    0
        small-r8_k8     363/7/12/559      5      1155 (512)    79216 (38653)     3516 (1975)     0
        pair-r64_k63    688/25/100/1267   14     6480 (1044)   372762 (78969)    19983 (4788)    0
        wide-r64_k63    1303/52/581/1319  24     7680 (2102)   393200 (139743)   31463 (9743)    0
        small-r64_k63   319/13/10/587     6      2880 (572)    165173 (40412)    10640 (2028)    0
        pair-r2_k64     787/24/100/1284   9      138 (1014)    14300 (80176)     19033 (4194)    0
        wide-r2_k64     1219/72/646/1456  27     408 (2167)    29002 (148428)    30224 (9731)    0
        small-r2_k64    345/14/22/525     6      103 (601)     8397 (44724)      11218 (2559)    0
        pair-nolife     787/24/100/1284   0      1014          80176             4194            31
        wide-nolife     1219/72/646/1456  0      2167          148428            9731            63
        small-nolife    345/14/22/525     0      601           44724             2559            24
        edge-r1_k0      620/0/12/543      3      0 (94)        279 (5495)        0 (219)         0
        edge-r64_k63    660/3/16/548      0      2760 (179)    121515 (9209)     4601 (717)      0

    At R = 64 every agent-step has cost > 0 (6480 = 18 * 6 * 60) and channel 4 covers every in-map cell of
    every window.  assert_inputs asserts the conditions these numbers meet, not the numbers."""
    assert_inputs(shape, params)
    run_random_case(case_name(shape, params), SHAPES[shape], path, cfg=PARAMS[params], obs_bits=packed,
                    **expectations(shape, params, path, packed))


# ------------------------------------------------------------------ the descent policy
def descent_env(params):
    def env_of(name, tuning=None, **kw):
        return H.case_env(SHAPES, name, DESCENT_SEED, tuning, cfg=PARAMS[params], **kw)
    return env_of


@functools.lru_cache(maxsize=None)
def descent_run(shape, params):
    """The oracle under tests/descent_ref.py's picks with PARAMS[params]; `on_goal`: the agents standing on
    their goals before each step."""
    steps = int(np.sum(LAUNCHES))

    def pick(oe, b, t, world):
        p, g = oe.agents()
        return descent_actions(oe.bfs(), p, t), dict(on_goal=(p == g).all(1))
    return H.oracle_rollout(SHAPES, shape, DESCENT_SEED, steps, set(np.cumsum(LAUNCHES).tolist()), pick, cfg=PARAMS[params])


@pytest.mark.parametrize("shape", ["pair", "wide"])
@pytest.mark.parametrize("params", ["costs", "nolife"])
def test_params_under_descent_match_oracle(shape, params):
    """mapf_rollout_descent into slot buffers, launches of 1 / 23 / 36 steps, every slot against the oracle;
    reward_total too (reward + goal_reward where a goal was reached, in float32).  Measured on the oracle
    (descent_run): goals reached 445 (pair-costs) and 424 (wide-costs), statuses -2 / -3 / -4 there 60 / 673 /
    431 and 104 / 2088 / 718 (descent never walks into an obstacle: no -1); with lifelong off no goal is
    reached and an agent stands on its goal in 4609 (pair) and 2546 (wide) agent-steps."""
    ref, state = descent_run(shape, params)
    goals, on_goal = int(ref["goals_reached"].sum()), int(ref["on_goal"].sum())
    counts = {s: int((ref["status"] == s).sum()) for s in (1, -1, -2, -3, -4)}
    print(f"{shape}-{params} descent: goals {goals}, on-goal agent-steps {on_goal}, statuses {counts}")
    if params == "costs":
        assert goals >= 20, goals
    else:
        assert goals == 0 and on_goal >= 20, (goals, on_goal)
    goal_reward = np.float32(PARAMS[params].get("goal_reward", 1.5))

    def reward_total(what, ref, t0, got, acts, which):
        for k, dt in which:
            t = t0 + dt
            want = np.where(ref["goals_reached"][t] == 1, ref["reward"][t] + goal_reward, ref["reward"][t])
            assert np.array_equal(got["reward_total"][k], want.astype(np.float32)), f"{what} t={t}: reward_total"

    mine = set()
    H.run_policy_case("descent", descent_env(params), mine, shape, "rollout", ref, state, LAUNCHES, hook=reward_total)
    (kname,) = mine
    assert kname.startswith("rollout_random_kernel<true,1," if shape == "pair" else "rollout_wide"), kname
