"""GPU parity of the per-step launch forms off their defaults.

include/mapf.h says of mapf_tuning: "these fields only pick between forms that produce identical
results".  The persistent rollout kernels' fields are swept in test_gpu_parity.py; here every field
of the per-step block (obs_envs, step_block, search_blocks, band_blocks, agent_lanes, serial_search,
no_defer) and xcd_remap / wide_overlap / wide_prio take values other than mapf_tuning_default's, and
few agents on large maps run at default tuning -- the shapes whose observe launch asked for several
times the LDS of a workgroup before mapf_create fitted obs_envs (tests/test_observe_lds_cpu.py).

Everything is exact: run_random_case / run_split_case (test_gpu_parity.py) compare every output,
observation and final state bit for bit with the C oracle and check the error counters.  One table,
FORMS, holds every form: the guard at the end reads it."""
import ctypes
import re

import pytest
import torch

from test_gpu_parity import FUSED_CASES, RANDOM_CASES, mk_env, run_random_case, run_split_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def short(case, steps=60, **kw):
    """An existing shape with fewer steps (a copy: the cases of test_gpu_parity.py keep theirs)."""
    c = dict(case)
    c["steps"] = min(steps, c["steps"])
    c.update(kw)
    return c


CASES = {
    # (a) few agents on large maps: 64 / N envs per workgroup would need 262 KB / 205 KB / 102 KB of
    # index images alone
    "n1_64x64_f7": dict(B=64, H=64, W=64, n=1, fov=7, nch=6, steps=30, map="rand"),
    "n2_80x80_f9": dict(B=32, H=80, W=80, n=2, fov=9, nch=6, steps=30, map="wh"),
    "n4_80x80_f11": dict(B=16, H=80, W=80, n=4, fov=11, nch=6, steps=30, map="rand", da=1, hp=1),
    # existing shapes, 60 steps at the most
    "n1_12x12_f7_looping": short(FUSED_CASES["n1_12x12_f7_looping"]),
    "n2_16x16_f9_dahp": short(FUSED_CASES["n2_16x16_f9_dahp"]),
    "c1_10x10_n4_f11": short(RANDOM_CASES["c1_10x10_n4_f11"]),
    "n7_24x24_f11_rand_dahp": short(FUSED_CASES["n7_24x24_f11_rand_dahp"]),
    "c2_20x20_n8_f11": short(RANDOM_CASES["c2_20x20_n8_f11"]),
    "r_n8_12x12_f11_deadlock": short(RANDOM_CASES["r_n8_12x12_f11_deadlock"], min_deadlocks=0),
    "dense_12x12_n16_f9_dahp": short(RANDOM_CASES["dense_12x12_n16_f9_dahp"]),
    "c5_80x80_n64_f11_bfsch": short(RANDOM_CASES["c5_80x80_n64_f11_bfsch"], steps=20),
    # (c) N = 8 at B = 9: with 64 threads one workgroup holds exactly one 64-lane (G = 8) env, nine workgroups
    "n8_20x20_f11_b9": short(RANDOM_CASES["c2_20x20_n8_f11"], steps=40, B=9),
    # (d) xcd_remap / wide_overlap / wide_prio on the rollout path, two 23-step launches.  The remap is the
    # identity unless the workgroup count is a multiple of 8.  Pair-lane, B = 64: plan_rollout_random
    # launches ceil(64 / 4) = 16 workgroups (ungrouped: 16 workgroups on >= 16 CUs are one per CU, not
    # four) -- a multiple of 8.  One wave per env, B = 12: plan_wide_t launches B / epw = 12 workgroups
    # (one env per workgroup while a CU holds one env) -- not a multiple.
    "x_n8_20x20_f11_b64": short(RANDOM_CASES["c2_20x20_n8_f11"], steps=46),
    "x_n16_40x40_f9_b12": short(RANDOM_CASES["c4_40x40_n16_f9_looping"], steps=46, B=12),
}
ROLLOUT_GRIDS = {"x_n8_20x20_f11_b64": (1, 16), "x_n16_40x40_f9_b12": (2, 12)}     # case -> (kernel kind, workgroups)

# the split-path shapes of test_split_path_back_to_back_steps_match_oracle: (B, H, n, fov, nch, steps)
SPLIT = {"c4_split_40x40_n16": (48, 40, 16, 9, 6, 40), "c5_split_80x80_n64_bfsch": (4, 80, 64, 11, 7, 20)}

FORMS = {}      # name -> (case, path, tuning); path: run_random_case's, or "split" / "split_bits" (run_split_case)


def form(case, path, **tuning):
    name = "-".join([case, path] + [f"{k}{v}" for k, v in tuning.items()])
    assert name not in FORMS
    FORMS[name] = (case, path, tuning)


# (a) default tuning
for _case in ("n1_64x64_f7", "n2_80x80_f9", "n4_80x80_f11"):
    for _path in ("plain", "fused", "rollout"):
        form(_case, _path)
# (b) the agent-per-lane step for N <= 8: step_kernel with Group(G), G = 1, 2, 4, 8 (8 also from N = 7)
for _case in ("n1_12x12_f7_looping", "n2_16x16_f9_dahp", "c1_10x10_n4_f11", "n7_24x24_f11_rand_dahp",
              "c2_20x20_n8_f11", "r_n8_12x12_f11_deadlock"):
    for _path in ("plain", "random", "fused"):
        form(_case, _path, agent_lanes=1)
# (c) threads per step workgroup.  Pair lanes: N = 7 at ragged B = 37, N = 8 at B = 9; agent lanes:
# N = 16 (four envs per wave) and c5's N = 64 at B = 3 (one wave per env: at 64 threads one env per workgroup)
for _blk in (64, 128):
    form("n7_24x24_f11_rand_dahp", "random", step_block=_blk)
    form("n8_20x20_f11_b9", "plain", step_block=_blk)
    form("dense_12x12_n16_f9_dahp", "random", step_block=_blk)
    form("c5_80x80_n64_f11_bfsch", "plain", step_block=_blk)
# (d) envs per observe workgroup: 3 and 5 do not divide B = 64; 64 is below (its own test: it may be refused)
for _e in (1, 3, 5):
    form("c2_20x20_n8_f11", "plain", obs_envs=_e)
form("dense_12x12_n16_f9_dahp", "plain", obs_envs=4)
form("c5_80x80_n64_f11_bfsch", "plain", obs_envs=2)             # BFS windows of two envs in LDS
# search workgroups of the observe / fused launch (W <= 32: hosted; human "random": A* at every path end)
for _s in (1, 1024):
    form("c2_20x20_n8_f11", "plain", search_blocks=_s)
    form("c2_20x20_n8_f11", "fused", search_blocks=_s)
# zero-band workgroups of the fused launch (c2: channel 5 is the band); with use_hp there is no band
for _z in (1, 7, 4096):
    form("c2_20x20_n8_f11", "fused", band_blocks=_z)
form("n2_16x16_f9_dahp", "fused", band_blocks=7)
# where the split path's search runs and when it is joined
for _t in (dict(serial_search=1), dict(no_defer=1), dict(serial_search=1, no_defer=1)):
    form("c4_split_40x40_n16", "split", **_t)
    form("c5_split_80x80_n64_bfsch", "split", **_t)
    form("c5_split_80x80_n64_bfsch", "split_bits", **_t)
# persistent kernels: env order, pipelining and priority
for _case in ROLLOUT_GRIDS:
    for _t in (dict(xcd_remap=0), dict(wide_overlap=0), dict(wide_prio=0)):
        form(_case, "rollout", **_t)


def expectations(case, path, tuning):
    """What the handle must report for a form, beyond the tuning it reads back."""
    kw = {}
    if case in ("n1_64x64_f7", "n2_80x80_f9", "n4_80x80_f11") or tuning.get("agent_lanes"):
        kw["expect_fused"] = False                       # mapf_step_observe falls back to step + observe
    if tuning.get("agent_lanes"):
        kw["expect_rollout_kernel"] = (0, 2)             # never the pair-lane rollout
    if "band_blocks" in tuning or ("search_blocks" in tuning and path == "fused"):
        kw["expect_fused"] = True                        # the one-launch kernel really takes these
    if case in ROLLOUT_GRIDS:
        kw["expect_rollout_kernel"] = ROLLOUT_GRIDS[case][0]
    return kw


@pytest.mark.parametrize("name", list(FORMS))
def test_form_matches_oracle(name):
    case, path, tuning = FORMS[name]
    if path in ("split", "split_bits"):
        run_split_case(name, *SPLIT[case], tuning=tuning, bits=path == "split_bits")
        return
    c = CASES[case]
    if case == "r_n8_12x12_f11_deadlock" and path != "random":
        c = dict(c, min_deadlocks=1)      # these two runs' 60 steps hold a fixActions deadlock (the oracle counts it)
    run_random_case(name, c, path, tuning=tuning or None, expect_tuning=tuning, **expectations(case, path, tuning))


@pytest.mark.parametrize("case", list(ROLLOUT_GRIDS))
def test_rollout_cases_launch_the_stated_workgroup_counts(case):
    """The cases of the xcd_remap forms: one workgroup count a multiple of 8 (the remap permutes the
    envs), one not (it is the identity), read from the library's own plan."""
    c = CASES[case]
    kind, grid = ROLLOUT_GRIDS[case]
    env = mk_env(B=c["B"], H=c["H"], W=c["W"], num_agents=c["n"], fov=c["fov"], num_channel=c["nch"],
                 human_mode=c.get("human", "random"), goal_mode="random", fix_choice=1, tuning=dict(xcd_remap=0))
    try:
        assert env.rollout_kernel == kind
        for slots in (False, True):
            plan = env.rollout_plan(slots)
            assert int(re.search(r" grid=(\d+)", plan).group(1)) == grid and " remap=0" in plan, plan
    finally:
        env.close()
    assert [g % 8 == 0 for _, g in ROLLOUT_GRIDS.values()] == [True, False]


def test_obs_envs_64_is_refused_unless_it_fits():
    """c2's shape with 64 envs per observe workgroup asks for ~80 KB of LDS (default: 8 envs, 11 KB).
    mapf_set_tuning takes it only where the device allows such a workgroup; otherwise MAPF_EINVAL,
    nothing changed, and the message names the largest value that fits -- which is then run."""
    from mapf_amd import _lib
    c = CASES["c2_20x20_n8_f11"]
    env = mk_env(B=c["B"], H=c["H"], W=c["W"], num_agents=c["n"], fov=c["fov"], num_channel=c["nch"])
    try:
        assert env.tuning()["obs_envs"] == 0
        need = int(_lib.lib().mapf_observe_lds(ctypes.byref(env.cfg), 64, 0, None))
        assert 65536 < need <= 163840
        envs = 64
        try:
            env.set_tuning(obs_envs=64)
        except RuntimeError as err:
            msg = str(err)
            assert "libmapf error -1" in msg and "obs_envs 64" in msg, msg
            limit = int(re.search(r"over the device's (\d+)", msg).group(1))
            envs = int(re.search(r"largest value that fits is (\d+)", msg).group(1))
            print(f"device LDS limit {limit}: obs_envs 64 refused, largest fitting {envs}")
            assert limit < need and 8 <= envs < 64
            fit = ctypes.c_int32()
            assert _lib.lib().mapf_observe_lds(ctypes.byref(env.cfg), 64, limit, ctypes.byref(fit)) <= limit
            assert fit.value == envs
            assert env.tuning()["obs_envs"] == 0              # nothing changed
        else:
            print(f"obs_envs 64 accepted: the device allows {need} bytes of LDS per workgroup")
    finally:
        env.close()
    run_random_case(f"c2_20x20_n8_f11-plain-obs_envs{envs}", c, "plain", tuning=dict(obs_envs=envs),
                    expect_tuning=dict(obs_envs=envs))


# ------------------------------------------------------------------------------------- guards
def guarded_fields():
    from mapf_amd import _lib
    f = _lib.TUNING_FIELDS
    return f[f.index("xcd_remap"):f.index("no_defer") + 1]


def test_every_per_step_field_has_a_form_off_its_default():
    """Every field of mapf_tuning from xcd_remap to no_defer occurs in FORMS with a value other than
    mapf_tuning_default's: a knob added there later fails this until it gets a form."""
    from mapf_amd.env import BatchedMapfGym
    default = BatchedMapfGym.default_tuning()
    fields = guarded_fields()
    assert {"xcd_remap", "obs_envs", "step_block", "search_blocks", "band_blocks", "agent_lanes", "serial_search",
            "no_defer"} <= set(fields)
    missing = [f for f in fields if not any(t.get(f, default[f]) != default[f] for _, _, t in FORMS.values())]
    assert not missing, missing
    for f in ("wide_overlap", "wide_prio"):
        assert any(t.get(f, default[f]) != default[f] for _, _, t in FORMS.values()), f


# one value outside each field's range (mapf.h: mapf_tuning)
OUT_OF_RANGE = dict(roll_occ=17, roll_group=2, roll_fair=-2, roll_slack=-2, wide_nt=2, wide_pipe=2, wide_grid=-1,
                    wide_overlap=2, wide_obs=3, wide_epw=13, wide_pair=2, wide_slack=-2, wide_fair=-1, wide_prio=2,
                    wide_bfsobs=2, xcd_remap=2, obs_envs=65, step_block=192, search_blocks=0, band_blocks=4097,
                    agent_lanes=2, serial_search=-1, no_defer=2, diag_exp=4)


def test_set_tuning_round_trip_and_rejections():
    """A valid struct reads back field for field; one out-of-range value per field is MAPF_EINVAL and
    leaves the previous struct in place."""
    from mapf_amd import _lib
    assert set(OUT_OF_RANGE) == set(_lib.TUNING_FIELDS)
    c = CASES["c2_20x20_n8_f11"]
    env = mk_env(B=c["B"], H=c["H"], W=c["W"], num_agents=c["n"], fov=c["fov"], num_channel=c["nch"])
    try:
        assert env.tuning() == env.default_tuning()
        valid = dict(roll_occ=3, roll_group=0, roll_fair=2, roll_slack=5, wide_nt=1, wide_pipe=0, wide_grid=0,
                     wide_overlap=0, wide_obs=1, wide_epw=4, wide_pair=1, wide_slack=-1, wide_fair=3, wide_prio=0,
                     wide_bfsobs=0, xcd_remap=0, obs_envs=5, step_block=128, search_blocks=17, band_blocks=9,
                     agent_lanes=1, serial_search=1, no_defer=1, diag_exp=2)
        assert set(valid) == set(_lib.TUNING_FIELDS)
        assert all(valid[k] != v for k, v in env.default_tuning().items())
        env.set_tuning(**valid)
        assert env.tuning() == valid
        for field, bad in OUT_OF_RANGE.items():
            t = _lib.Tuning(**valid)
            setattr(t, field, bad)
            assert _lib.lib().mapf_set_tuning(env.h, ctypes.byref(t)) == -1, field
            assert _lib.lib().mapf_last_error(), field
            assert env.tuning() == valid, field
    finally:
        env.close()
