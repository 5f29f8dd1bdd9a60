"""GPU: sparse slot-buffer rollouts (mapf_rollout_sparse, include/mapf.h; BatchedMapfGym.rollout_sparse and
the default rollout_launcher).

A piece is 16 consecutive floats of an env's observation slice in one slot; the caller's shadow holds one
bit per piece.  A launch stores, for the slots the caller vouches for, exactly the pieces that the shadow
names or that hold a non-zero now, and leaves the slots' new masks.  Every case runs an unflagged twin env
beside the env under test and compares bit for bit: launch 1 (valid = 0) on NaN-filled buffers equals the
twin; after filling `obs` with 7.0, launch 2 (valid = T) keeps 7.0 exactly in the pieces that are all zero
in the twin's launch-1 and launch-2 observations; launch 3 (valid = 2) mixes both kinds of step.  The
shadow after each launch is the numpy mask of the twin's observations."""
import numpy as np
import pytest
import torch

from test_gpu_parity import assert_no_errors, build_maps, mk_env

pytestmark = pytest.mark.gpu

T = 5
GROUPED = dict(roll_occ=4, roll_group=1)
# name: map side, fov, B, tuning, the kernel's SUBS, policy.  Grouped sparse launches run with priority by
# progress (roll_fair auto = 4); one case paces them instead.  B: a full group (64), a partial group (61: the
# last quarter holds one env), a partial quarter (5)
CASES = {
    "s20_f11_b64_random": (20, 11, 64, GROUPED, 4, "random"),
    "s20_f11_b61_tape": (20, 11, 61, GROUPED, 4, "tape"),
    "s20_f11_b64_random_paced": (20, 11, 64, dict(GROUPED, roll_fair=0), 4, "random"),    # the band form's pacing
    "s10_f11_b61_pibt": (10, 11, 61, GROUPED, 4, "pibt"),
    "s10_f3_b64_descent": (10, 3, 64, GROUPED, 4, "descent"),
    "s10_f3_b5_descent": (10, 3, 5, None, 1, "descent"),
    "s20_f3_b64_pibt": (20, 3, 64, None, 1, "pibt"),
    "s20_f11_b5_random": (20, 11, 5, None, 1, "random"),
    "s10_f11_b5_tape": (10, 11, 5, None, 1, "tape"),
}
N, C = 8, 6


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def pair(side, fov, B, tuning, n=N, **kw):
    """The env under test and its twin, reset alike."""
    case = dict(H=side, W=side, map="wh")
    maps, shared = build_maps(case, B, np.random.default_rng(5))
    envs = []
    for _ in range(2):
        env = mk_env(B=B, H=side, W=side, num_agents=n, fov=fov, num_channel=C, human_mode="random", goal_mode="random",
                     fix_choice=1, shared_map=shared, seed=0x5BA45E, env_offset=3, tuning=tuning, **kw)
        env.reset_seeded(maps)
        envs.append(env)
    return envs


def buffers(env, steps=T):
    B, n, f = env.B, env.N, env.F
    return dict(actions=torch.full((steps, B, n), -9, dtype=torch.int32, device=env.device),
                obs=torch.full((steps, B, n, C, f, f), float("nan"), device=env.device),
                vec=torch.full((steps, B, n, 4), float("nan"), device=env.device),
                out={key: torch.full((steps,) + tuple(v.shape), -7, dtype=v.dtype, device=env.device)
                     for key, v in env.out.items()})


def refill(roll, obs_value):
    roll["obs"].fill_(obs_value)
    roll["vec"].fill_(float("nan"))
    roll["actions"].fill_(-9)
    for v in roll["out"].values():
        v.fill_(-7)


def piece_nonzero(obs):
    """bool [steps, B, pieces]: the 16-float pieces of every env-slot that hold a non-zero."""
    steps, B = obs.shape[:2]
    return (obs.reshape(steps, B, -1, 16) != 0).any(axis=3)


def mask_words(nz):
    """The shadow of piece_nonzero's array: uint32 [steps, B, 16], bit p of the 16 words = piece p."""
    steps, B, pieces = nz.shape
    bits = np.zeros((steps, B, 512), np.uint64)
    bits[:, :, :pieces] = nz
    return (bits.reshape(steps, B, 16, 32) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32)


def tape_of(env, k):
    g = torch.Generator().manual_seed(100 + k)
    return torch.randint(0, 5, (T, env.B, env.N), generator=g, dtype=torch.int32).to(env.device)


def launch_pair(env, twin, policy, k, roll, ref, shadow, valid):
    """Launch k of both envs; returns the twin's observations as a numpy array."""
    kw = dict(tape=tape_of(env, k)) if policy == "tape" else {}
    env.rollout_sparse(T, policy, shadow=shadow, valid=valid, actions=roll["actions"], obs=roll["obs"], vec=roll["vec"],
                       out=roll["out"], **kw)
    twin.rollout(T, policy, slots=True, actions=ref["actions"], obs=ref["obs"], vec=ref["vec"], out=ref["out"], **kw)
    torch.cuda.synchronize()
    return ref["obs"].cpu().numpy()


def check(name, k, roll, ref, policy, keep=None):
    """Everything equals the twin's, except that the pieces of `keep` (bool [T, B, pieces]) hold 7.0."""
    want = ref["obs"].cpu().numpy().copy()
    if keep is not None:
        want.reshape(keep.shape + (16,))[keep] = 7.0
    got = roll["obs"].cpu().numpy()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{name} launch {k}: {len(bad)} obs floats differ, first (t, b, agent, ch, y, x) = {bad[0]}"
    assert torch.equal(roll["vec"].view(torch.int32), ref["vec"].view(torch.int32)), f"{name} launch {k}: vec"
    if policy != "tape":
        assert torch.equal(roll["actions"], ref["actions"]), f"{name} launch {k}: actions"
    for key in ref["out"]:
        assert torch.equal(roll["out"][key], ref["out"][key]), f"{name} launch {k}: {key}"


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_launches_store_exactly_the_pieces_that_change(name):
    side, fov, B, tuning, subs, policy = CASES[name]
    env, twin = pair(side, fov, B, tuning)
    try:
        roll, ref = buffers(env), buffers(twin)
        tag = "" if policy == "random" else "," + policy
        assert env.rollout_sparse_plan(roll["obs"], policy).split(" ")[0] == \
            "rollout_random_kernel<true,%d,sparse64%s>" % (subs, tag)
        shadow = torch.full((T, B, 16), 0x5A5A5A5A, dtype=torch.int32, device=env.device)    # valid = 0: not read
        obs1 = launch_pair(env, twin, policy, 0, roll, ref, shadow, 0)
        check(name, 0, roll, ref, policy)
        nz1 = piece_nonzero(obs1)
        assert np.array_equal(shadow.cpu().numpy().view(np.uint32), mask_words(nz1)), f"{name}: shadow after launch 1"
        assert nz1.any() and not nz1.all()                  # both kinds of piece occur

        refill(roll, 7.0)
        refill(ref, float("nan"))
        nz2 = piece_nonzero(launch_pair(env, twin, policy, 1, roll, ref, shadow, T))
        check(name, 1, roll, ref, policy, keep=~(nz1 | nz2))
        assert np.array_equal(shadow.cpu().numpy().view(np.uint32), mask_words(nz2)), f"{name}: shadow after launch 2"

        refill(roll, 7.0)
        refill(ref, float("nan"))
        nz3 = piece_nonzero(launch_pair(env, twin, policy, 2, roll, ref, shadow, 2))
        keep = ~(nz2 | nz3)
        keep[2:] = False                                     # steps past `valid` store every float
        check(name, 2, roll, ref, policy, keep=keep)
        assert np.array_equal(shadow.cpu().numpy().view(np.uint32), mask_words(nz3)), f"{name}: shadow after launch 3"
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()
        twin.close()


def test_where_the_form_does_not_apply_the_launch_is_the_band_one():
    """N = 6, FOV 9: an env's slice is 2,916 floats, no whole number of pieces.  The plan says band64,
    valid = 0 stores everything, valid = T leaves alone nothing but floats of the zero band (channel 5),
    and the shadow is not touched."""
    env, twin = pair(16, 9, 37, None, n=6)
    try:
        roll, ref = buffers(env), buffers(twin)
        plan = env.rollout_sparse_plan(roll["obs"])
        assert plan.split(" ")[0] == "rollout_random_kernel<true,1,band64>", plan
        shadow = torch.full((T, 37, 16), 0x5A5A5A5A, dtype=torch.int32, device=env.device)
        launch_pair(env, twin, "random", 0, roll, ref, shadow, 0)
        check("n6_f9", 0, roll, ref, "random")
        refill(roll, 7.0)
        refill(ref, float("nan"))
        launch_pair(env, twin, "random", 1, roll, ref, shadow, T)
        got, want = roll["obs"].cpu().numpy(), ref["obs"].cpu().numpy()
        kept = got.view(np.uint32) != want.view(np.uint32)
        assert kept.any() and not kept[:, :, :, :5].any() and (got[kept] == 7.0).all()
        assert (want[:, :, :, 5] == 0).all()
        assert torch.equal(roll["vec"].view(torch.int32), ref["vec"].view(torch.int32))
        assert (shadow == 0x5A5A5A5A).all()
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()
        twin.close()


def test_launcher_calls_with_no_writes_in_between_equal_the_twin():
    env, twin = pair(20, 11, 64, GROUPED)
    try:
        roll, ref = buffers(env), buffers(twin)
        launch = env.rollout_launcher(T, slots=True, **roll)
        assert launch.sparse.valid == 0
        for call in range(3):
            launch()
            twin.rollout(T, "random", slots=True, **ref)
            torch.cuda.synchronize()
            check("launcher", call, roll, ref, "random")
            assert launch.sparse.valid == T
        nz = piece_nonzero(ref["obs"].cpu().numpy())
        assert np.array_equal(launch.sparse.shadow[:T].cpu().numpy().view(np.uint32), mask_words(nz))
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()
        twin.close()


def test_two_launchers_of_different_lengths_over_one_buffer_equal_the_twin():
    short = 3
    env, twin = pair(20, 11, 61, GROUPED)
    try:
        roll, ref = buffers(env), buffers(twin)
        head = lambda r, n: dict(actions=r["actions"][:n], obs=r["obs"][:n], vec=r["vec"][:n],
                                 out={k: v[:n] for k, v in r["out"].items()})
        first, second = env.rollout_launcher(short, slots=True, **head(roll, short)), env.rollout_launcher(T, slots=True, **roll)
        assert first.sparse is second.sparse
        for call, (launch, n) in enumerate([(first, short), (second, T), (first, short), (second, T)]):
            launch()
            twin.rollout(n, "random", slots=True, **head(ref, n))
            torch.cuda.synchronize()
            assert first.sparse.valid == (short if call == 0 else T)
            if call:
                check("two launchers", call, roll, ref, "random")
            else:       # the slots past the short launcher's are still NaN in both
                check("two launchers", call, head(roll, short), head(ref, short), "random")
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()
        twin.close()
