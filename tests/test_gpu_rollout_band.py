"""GPU: slot-buffer rollouts launched with MAPF_SLOTS_BAND_CLEAN (include/mapf.h).

The caller promises that the zero band of every slot (channel 5 while use_hp is off) already holds
zeros; the pair-lane kernel then leaves out exactly the stores mapf_obs_band_skip names and writes
everything else as before.  Each case: NaN-filled buffers, one launch without the bit (every float
bit-exact vs the oracle), then sentinels (7.0 in the band, NaN elsewhere) and one launch with the
bit on the oracle's next 23 steps: a band float keeps its 7.0 exactly where the host bitmap says
"skipped" and is 0.0 elsewhere, every other float and every step output is the oracle's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_parity import GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, assert_no_errors, build_maps, host, mk_env

pytestmark = pytest.mark.gpu

T = 23
OUT_KEYS = [("status", "status"), ("reward", "reward"), ("cost", "cost"), ("train_valid", "valid"),
            ("actions_fixed", "fixed"), ("goals_reached", "goals"), ("constraints", "constr"), ("shadow_goals", "shadow")]
CASES = {
    "b64": GROUP_CASES["g_n8_20x20_f11"],                    # both env parities (an env is 181.5 lines)
    "b61": GROUP_CASES["g_n8_20x20_f11_ragged61"],           # the last group's last quarter holds one env
    "b37_n6_f9": dict(ROLLOUT_CASES["r_n6_16x16_f9_dahp"], da=0, hp=0),   # slot stride % 64 != 0: the set moves with t
    "b45_dahp": GROUP_CASES["g_n6_16x16_f9_dahp_ragged"],    # use_hp on: no band
    "c4_wide": RANDOM_CASES["c4_40x40_n16_f9_looping"],      # the one-wave-per-env kernel: stores everything
}
LAUNCHES = {"b64": 3}                # launches of T steps the oracle runs ahead (default 2); b64: the launcher test's 3
FORMS = {"cu_group": dict(roll_occ=4, roll_group=1), "default": None}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def setup(name):
    case = CASES[name]
    maps, shared = build_maps(case, case["B"], np.random.default_rng(5))
    return case, maps, shared, 0x5EED0000 + len(name)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's first LAUNCHES * T steps of the case, computed once and shared by the tests
    (read-only): actions, observations, vectors and step outputs as [steps, B, ...] arrays."""
    launches = LAUNCHES.get(name, 2)
    case, maps, shared, seed = setup(name)
    B, n = case["B"], case["n"]
    cfg = O.make_config(case["H"], case["W"], n, case["fov"], case["nch"], use_da=case.get("da", 0),
                        use_hp=case.get("hp", 0), human_mode={"random": 1, "looping": 0}[case.get("human", "random")],
                        goal_mode=1, fix_choice=1, seed=seed, env_offset=7)
    rows = []
    for b in range(B):
        oe = O.OracleEnv(cfg, env_id=7 + b)
        oe.reset_random(maps if shared else maps[b])
        steps = []
        for _ in range(launches * T):
            a = oe.random_actions()
            o = oe.step(a)
            oo, ov = oe.observe()
            steps.append(dict(actions=np.array(a), obs=oo, vec=ov, **{k: np.array(o[key]) for k, key in OUT_KEYS}))
        assert oe.errors() == 0
        rows.append(steps)
    ref = {k: np.stack([np.stack([rows[b][t][k] for b in range(B)]) for t in range(launches * T)])
           for k in rows[0][0]}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def fresh_buffers(env, case):
    B, n, nch, fov = case["B"], case["n"], case["nch"], case["fov"]
    return dict(actions=torch.full((T, B, n), -9, dtype=torch.int32, device=env.device),
                obs=torch.full((T, B, n, nch, fov, fov), float("nan"), device=env.device),
                vec=torch.full((T, B, n, 4), float("nan"), device=env.device),
                out={key: torch.full((T,) + tuple(v.shape), -7, dtype=v.dtype, device=env.device)
                     for key, v in env.out.items()})


def set_sentinels(roll):
    roll["obs"].fill_(float("nan"))
    roll["obs"][:, :, :, 5] = 7.0
    roll["vec"].fill_(float("nan"))
    roll["actions"].fill_(-9)
    for v in roll["out"].values():
        v.fill_(-7)


def host_skip(env, case, roll, expect_band):
    """bool [T, B, N*C*F*F]: the floats a flagged launch into roll["obs"] leaves alone, from the host
    side of the kernel's own skip function at every slot's and env's address."""
    from mapf_amd import _lib
    B, n, nch, fov = case["B"], case["n"], case["nch"], case["fov"]
    env_floats = n * nch * fov * fov
    band = np.zeros((n, nch, fov * fov), bool)
    band[:, 5] = True
    by_off = {}
    skip = np.zeros((T, B, env_floats), bool)
    for t in range(T):
        for b in range(B):
            off = (roll["obs"].data_ptr() + (t * B + b) * env_floats * 4) % 128
            if off not in by_off:
                buf = np.zeros(env_floats // 4, np.uint8)
                assert _lib.lib().mapf_obs_band_skip(ctypes.byref(env.cfg), 0, off, buf.ctypes.data, len(buf)) == len(buf)
                by_off[off] = np.repeat(buf.astype(bool), 4)
                assert not (by_off[off] & ~band.reshape(-1)).any()
            skip[t, b] = by_off[off]
    if expect_band:       # a band of L bytes holds at least (L - 60) // 64 whole 64-B pieces whatever its
        #                   alignment: 6 of F = 11's 484 B, 4 of F = 9's 324 B -- over 3/4 of the band
        assert skip.sum() >= 0.75 * T * B * n * fov * fov, skip.sum()
    else:
        assert not skip.any()
    return skip


def check_launch(name, ref, k, roll, skip=None):
    """Launch k's buffers against the oracle's steps [k*T, (k+1)*T); skip: floats that keep the sentinel."""
    sl = slice(k * T, (k + 1) * T)
    got = dict(actions=roll["actions"].cpu().numpy(), vec=roll["vec"].cpu().numpy(), **host(roll["out"]))
    for key in ["actions", "vec"] + [k_ for k_, _ in OUT_KEYS]:
        want = ref[key][sl].astype(got[key].dtype).reshape(got[key].shape)
        assert np.array_equal(got[key], want), f"{name} launch {k}: {key}"
    obs = roll["obs"].cpu().numpy()
    want = ref["obs"][sl].reshape(obs.shape).copy()
    if skip is not None:
        want.reshape(skip.shape)[skip] = 7.0
    bad = np.argwhere(obs.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{name} launch {k}: {len(bad)} obs floats differ, first (t, b, agent, ch, y, x) = {bad[0]}"


def run_case(name, tuning, expect_kind, expect_band, expect_plan=None):
    """expect_band True: the host bitmap's floats keep the sentinel; False: the host bitmap is empty
    (no band); None: the launch stores everything whatever the bitmap says (not the pair-lane kernel)."""
    case, maps, shared, seed = setup(name)
    env = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 use_da=case.get("da", 0), use_hp=case.get("hp", 0), human_mode=case.get("human", "random"),
                 goal_mode="random", fix_choice=1, shared_map=shared, seed=seed, env_offset=7, tuning=tuning)
    try:
        env.reset_seeded(maps)
        assert env.rollout_kernel == expect_kind
        if expect_plan is not None:
            assert env.rollout_plan(slots=True, band_clean=True).split(" ")[0] == expect_plan
        ref = oracle_run(name)
        roll = fresh_buffers(env, case)
        env.rollout_random(T, slots=True, **roll)                       # launch 1: no bit, every float written
        check_launch(name, ref, 0, roll)
        set_sentinels(roll)
        env.rollout_random(T, slots=True, band_clean=True, **roll)      # launch 2: the band is declared clean
        check_launch(name, ref, 1, roll, None if expect_band is None else host_skip(env, case, roll, expect_band))
        assert_no_errors(env)
    finally:
        env.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["b64", "b61", "b37_n6_f9"])
def test_clean_band_launch_skips_exactly_the_host_bitmap(name, form):
    sub = 4 if form == "cu_group" and CASES[name]["B"] > 60 else 1      # B = 37: 10 workgroups, no CU groups
    run_case(name, FORMS[form], 1, True, expect_plan="rollout_random_kernel<true,%d,band64>" % sub)


@pytest.mark.parametrize("form", list(FORMS))
def test_no_band_with_use_hp_everything_is_stored(form):
    run_case("b45_dahp", FORMS[form], 1, False)


def test_wide_kernel_ignores_the_bit():
    run_case("c4_wide", None, 2, None)


def test_launcher_declares_the_band_clean_after_its_first_call_until_invalidated():
    name = "b64"
    case, maps, shared, seed = setup(name)
    env = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared, seed=seed, env_offset=7,
                 tuning=FORMS["cu_group"])
    try:
        env.reset_seeded(maps)
        ref = oracle_run(name)
        roll = fresh_buffers(env, case)
        launch = env.rollout_launcher(T, slots=True, **roll)
        launch()                                                        # call 1 overwrites the NaNs completely
        check_launch(name, ref, 0, roll)
        set_sentinels(roll)
        launch()                                                        # call 2 leaves the band's sentinels
        check_launch(name, ref, 1, roll, host_skip(env, case, roll, True))
        set_sentinels(roll)
        launch.invalidate()
        launch()                                                        # call 3 stores everything again
        check_launch(name, ref, 2, roll)
        assert_no_errors(env)
    finally:
        env.close()
