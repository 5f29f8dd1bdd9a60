"""GPU: bit-packed observations, one bit per cell (include/mapf.h, "Packed observations").

The observing kernels' OBS_BITS instantiations store an agent's [C][F][F] block of 0/1 floats as
WPA = ceil(C*F*F / 32) uint32 words.  Every case prefills its packed buffer with 0xFFFFFFFF (and its
float buffers with NaN) and compares every word with the numpy definition of the format applied to the
CPU oracle's observation -- or to a float twin handle's -- bit for bit; nothing here has a tolerance.
The oracle runs are the tape file's (tests/test_gpu_rollout_tape.py: oracle_run, shared and read-only).

The default packed plans' kernels that this file compared against the oracle are recorded in
BITS_COVERED; tests/test_gpu_obs_bits_policy.py ends with the guard over the BASELINE presets.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_rollout_tape as tape_tests
from kernel_registry import record_rollout_kernel
from rollout_harness import OUT_KEYS, check_state, preset_envs, slot_buffers
from test_gpu_parity import FUSED_CASES, assert_no_errors, host
from test_gpu_rollout_tape import LAUNCHES, PAIR_CASES, case_env, case_setup, make_tape, oracle_run
from test_obs_bits_cpu import pack_np

pytestmark = pytest.mark.gpu

tape_tests.CASES.setdefault("n1_12x12_f7_looping", FUSED_CASES["n1_12x12_f7_looping"])   # a fused per-step case
BITS_COVERED = set()          # packed kernel names compared against the oracle in this session


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def words(t):
    """A packed device buffer as host uint32."""
    return t.cpu().numpy().view(np.uint32)


def bits_buffers(env, k, lead=True):
    """slot_buffers with the packed observation buffer, every word 0xFFFFFFFF."""
    buf = slot_buffers(env, k)
    shape = ((k,) if lead else ()) + (env.B, env.N, env.obs_words)
    buf["obs"] = torch.full(shape, -1, dtype=torch.int32, device=env.device)
    return buf


def want_bits(env, obs):
    return pack_np(obs, env.C, env.F).reshape(env.B, env.N, env.obs_words)


def check_packed(what, env, ref, t0, got_out, bits, vec, slots):
    """check_slots of the tape file with the packed observation: [(slot index, step relative to t0)]."""
    bits, vec = words(bits), vec.cpu().numpy()
    for k, dt in slots:
        t = t0 + dt
        for key, _ in OUT_KEYS:
            want = ref[key][t].astype(got_out[key].dtype).reshape(got_out[key][k].shape)
            assert np.array_equal(got_out[key][k], want), f"{what} t={t}: {key}"
        want = ref["vec"][t].astype(np.float32).reshape(vec[k].shape)
        assert np.array_equal(vec[k].view(np.uint32), want.view(np.uint32)), f"{what} t={t}: vec"
        bad = np.argwhere(bits[k] != want_bits(env, ref["obs"][t]))
        assert len(bad) == 0, f"{what} t={t}: {len(bad)} packed words differ, first (b, agent, word) = {bad[0]}"


# ------------------------------------------------------------------ 1. per-step calls
# (name, step_observe is one fused launch -- None: not asserted, 300 single-agent envs per workgroup pass the
# fused form's LDS --, steps of the shared oracle run)
PER_STEP = [("r_n6_16x16_f9_dahp", True, 156), ("c2_20x20_n8_f11", True, 24), ("n1_12x12_f7_looping", None, 24),
            ("dense_12x12_n16_f9_dahp", False, 91), ("w_n20_48x90_f11_bfsch", False, 91)]


@pytest.mark.parametrize("name,fused,steps", PER_STEP)
def test_observe_bits_and_step_observe_bits_match_oracle(name, fused, steps):
    """24 steps of step_observe_bits, each followed by observe_bits into a second buffer: both equal the
    packed oracle observation.  fused: one step+observe launch; else step, search, observe launches --
    w_n20 has the BFS channel, where the float call forks the search and fixes channel 6 up as floats:
    the packed call joins the search first."""
    T = 24
    tape_h, ref, state = oracle_run(name, steps)
    env, case, _, _, _ = case_env(name)
    try:
        assert fused is None or env.fused == fused, name
        tape = torch.from_numpy(tape_h).to(env.device)
        for t in range(T):
            buf, again = bits_buffers(env, 1, lead=False), bits_buffers(env, 1, lead=False)
            out, bits, vec = env.step_observe_bits(tape[t], buf["obs"], buf["vec"][0], out={k: v[0] for k, v in buf["out"].items()})
            env.observe_bits(again["obs"], again["vec"][0])
            got = host(buf["out"])
            check_packed(f"{name} step_observe_bits", env, ref, t, got, bits[None], buf["vec"], [(0, 0)])
            assert np.array_equal(words(again["obs"]), words(bits)), f"t={t}: observe_bits"
            assert torch.equal(again["vec"].view(torch.int32), buf["vec"].view(torch.int32)), f"t={t}: observe_bits vec"
        check_state(env, state[T], name)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()


# ------------------------------------------------------------------ 2. rollouts on the tape policy
def run_bits_case(name, path, tuning=None, launches=LAUNCHES, expect=None, family=None):
    """run_tape_case of the tape file with obs_bits: "rollout" into [T]-slot buffers, "inplace" each
    launch's last step, "inplace1" one-step launches in place."""
    total = int(np.sum(launches))
    if path == "inplace1":
        launches = (1,) * 24
    elif path == "inplace":
        launches = launches[1:]
    tape_h, ref, state = oracle_run(name, total)
    env, case, _, _, _ = case_env(name, tuning)
    try:
        slots = path == "rollout"
        kname = env.rollout_actions_kernel_name(slots=slots, obs_bits=True)
        plain = env.rollout_actions_kernel_name(slots=slots)
        assert kname.endswith(",bits,tape>") and ",bits" not in plain, (kname, plain)
        if expect is not None:
            assert kname == expect, env.rollout_actions_plan(slots=slots, obs_bits=True)
        if family is not None:
            assert kname.startswith(family + "<"), env.rollout_actions_plan(slots=slots, obs_bits=True)
        # the band flag changes nothing in a packed plan
        assert env.rollout_actions_plan(slots, True, True) == env.rollout_actions_plan(slots, False, True)
        tape = torch.from_numpy(tape_h).to(env.device)
        t0 = 0
        for T in launches:
            buf = bits_buffers(env, T if slots else 1)
            if not slots:
                buf["obs"] = buf["obs"][0]
            env.rollout_actions(tape[t0:t0 + T], slots=slots, obs_bits=True, **buf)
            got = host(buf["out"])
            what = f"{name} {path} packed launch [{t0}, {t0 + T})"
            bits = buf["obs"] if slots else buf["obs"][None]
            check_packed(what, env, ref, t0, got, bits, buf["vec"], [(k, k) for k in range(T)] if slots else [(0, T - 1)])
            t0 += T
            check_state(env, state[t0], what)
        assert_no_errors(env, allow=(1, 2))
        BITS_COVERED.add(kname)
        record_rollout_kernel(kname, f"{name} {path} packed tape vs oracle")
    finally:
        env.close()


@pytest.mark.parametrize("path", ["rollout", "inplace1", "inplace"])
@pytest.mark.parametrize("name,tuning,subs", PAIR_CASES)
def test_pair_lane_packed_rollout_matches_oracle(name, tuning, subs, path):
    """Ungrouped ragged B = 37, grouped paced B = 61, grouped fair.  The plan without the flag is
    today's text, with it ",bits" follows the group count."""
    env = case_env(name, tuning)[0]
    try:
        slots = path == "rollout"
        assert env.rollout_actions_kernel_name(slots=slots) == "rollout_random_kernel<%s,%s,tape>" % ("true" if slots else "false", subs)
    finally:
        env.close()
    run_bits_case(name, path, tuning, expect="rollout_random_kernel<%s,%s,bits,tape>" % ("true" if path == "rollout" else "false", subs))


WIDE_BITS_CASES = [("c4_40x40_n16_f9_looping", None, "rollout", "rollout_wide3_kernel"),
                   ("c4_40x40_n16_f9_looping", None, "inplace", "rollout_wide3_kernel"),      # the last-step re-store
                   ("c4_40x40_n16_f9_looping", dict(wide_obs=1), "rollout", "rollout_wide_kernel"),
                   ("c4_40x40_n16_f9_looping", dict(wide_pipe=0), "rollout", "rollout_wide_kernel"),
                   ("c1_10x10_n4_f11", None, "rollout", None),
                   ("c1_10x10_n4_f11", None, "inplace", None),
                   ("c1_10x10_n4_f11", None, "inplace1", None),
                   ("c5_80x80_n64_f11_bfsch", None, "rollout", "rollout_wide_kernel"),
                   ("w_n20_48x90_f11_bfsch", None, "rollout", None)]


@pytest.mark.parametrize("name,tuning,path,family", WIDE_BITS_CASES)
def test_wide_packed_rollout_matches_oracle(name, tuning, path, family):
    """The one-wave-per-env kernels, launches of 1, 23 and 67 steps: three waves per env into slots and
    in place (whose last step's observation is stored twice), two, one, u32 / u64 / 128-bit rows, the
    BFS channel.  Packed launches use plain stores: the name's store field reads false."""
    run_bits_case(name, path, tuning, launches=LAUNCHES[:3], family=family)
    env = case_env(name, tuning)[0]
    try:
        assert ",false,bits,tape>" in env.rollout_actions_kernel_name(path == "rollout", obs_bits=True)
    finally:
        env.close()


# ------------------------------------------------------------------ 3. the other policies against a float twin
def assert_twins_equal(a, b, fa, fb, what):
    """Packed launch `a` (buffers fa) against float launch `b` (buffers fb)."""
    torch.cuda.synchronize()
    want = pack_np(fb["obs"].cpu().numpy(), a.C, a.F).reshape(words(fa["obs"]).shape)
    assert np.array_equal(words(fa["obs"]), want), f"{what}: pack(float obs) != bits"
    assert torch.equal(fa["vec"].view(torch.int32), fb["vec"].view(torch.int32)), f"{what}: vec"
    for key in fa["out"]:
        assert torch.equal(fa["out"][key], fb["out"][key]), f"{what}: {key}"
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{what}: state {key}")
    assert torch.equal(a.bfs(), b.bfs()), f"{what}: bfs"
    assert (a.counters()[:8] == b.counters()[:8]).all(), what


def twin_envs(name, **kw):
    case, maps, shared, seed = case_setup(name)
    envs = []
    for _ in range(2):
        e = tape_tests.mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"],
                              num_channel=case["nch"], use_da=case.get("da", 0), use_hp=case.get("hp", 0),
                              human_mode=case.get("human", "random"), goal_mode="random", fix_choice=1, shared_map=shared,
                              seed=seed, env_offset=7, **kw)
        e.reset_seeded(maps)
        envs.append(e)
    return envs


@pytest.mark.parametrize("slots", [True, False])
@pytest.mark.parametrize("policy", ["random", "descent"])
@pytest.mark.parametrize("name", ["r_n6_16x16_f9_dahp", "c4_40x40_n16_f9_looping"])
def test_random_and_descent_packed_equal_a_float_twin(name, policy, slots):
    T = 40
    a, b = twin_envs(name)
    try:
        k = T if slots else 1
        fa, fb = bits_buffers(a, k), slot_buffers(b, k)
        acts = [torch.full((k, e.B, e.N), -9, dtype=torch.int32, device=e.device) for e in (a, b)]
        fn = "rollout_random" if policy == "random" else "rollout_descent"
        name_fn = a.rollout_kernel_name if policy == "random" else a.rollout_descent_kernel_name
        assert ",bits" in name_fn(slots, obs_bits=True) and ",bits" not in name_fn(slots)
        getattr(a, fn)(T, slots=slots, actions=acts[0], obs_bits=True, **fa)
        getattr(b, fn)(T, slots=slots, actions=acts[1], **fb)
        assert_twins_equal(a, b, fa, fb, f"{name} {policy} slots={slots}")
        assert torch.equal(acts[0], acts[1]) and int(acts[0].min()) >= 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. full size
@pytest.mark.parametrize("cfg", ["c2", "c4", "c5"])
def test_full_size_packed_slots_equal_the_float_buffer(cfg):
    """The BASELINE presets, T = 8 into slots on a packed and a float handle: the unpacked bits are the
    float buffer, and the packed buffer is exactly T*B*N*WPA*4 bytes."""
    from mapf_amd.env import unpack_obs
    T = 8
    a, b = preset_envs(cfg, 2)
    try:
        fa, fb = bits_buffers(a, T), slot_buffers(b, T)
        acts = [torch.full((T, e.B, e.N), -9, dtype=torch.int32, device=e.device) for e in (a, b)]
        a.rollout_random(T, slots=True, actions=acts[0], obs_bits=True, **fa)
        b.rollout_random(T, slots=True, actions=acts[1], **fb)
        torch.cuda.synchronize()
        wpa = {"c2": 23, "c4": 16, "c5": 27}[cfg]
        assert a.obs_words == wpa and fa["obs"].nbytes == T * a.B * a.N * wpa * 4
        assert fa["obs"].nbytes * 26 < fb["obs"].nbytes
        got = unpack_obs(fa["obs"], a.C, a.F)
        assert torch.equal(got.view(torch.int32), fb["obs"].view(torch.int32)), "unpacked bits != float obs"
        pad = 32 * wpa - a.C * a.F * a.F                  # padding bits written as 0 over the 0xFFFFFFFF prefill
        assert pad == 0 or not bool(((fa["obs"][..., -1] >> (32 - pad)) != 0).any())
        assert torch.equal(fa["vec"].view(torch.int32), fb["vec"].view(torch.int32))
        assert torch.equal(acts[0], acts[1])
        for key in fa["out"]:
            assert torch.equal(fa["out"][key], fb["out"][key]), key
        BITS_COVERED.add("full:" + a.rollout_kernel_name(True, obs_bits=True))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. the per-step fallback
@pytest.mark.parametrize("slots", [True, False])
def test_packed_rollout_without_a_one_launch_form_equals_the_per_step_calls(slots):
    """16 agents with the HP channel and k_predict = 64 have no one-launch kernel: the packed rollout
    issues T packed per-step launches, slot t at t * B*N*WPA words."""
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    name, T = "dense_12x12_n16_f9_dahp", 12
    case, maps, shared, seed = case_setup(name)
    envs = []
    for _ in range(2):
        cfg = make_config(case["B"], case["H"], case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                          use_da=1, use_hp=1, human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared,
                          seed=seed, env_offset=7)
        cfg.k_predict = 64
        envs.append(BatchedMapfGym(cfg))
        envs[-1].reset_seeded(maps)
    env, twin = envs
    try:
        assert not env.rollout_fused and env.rollout_actions_plan(slots, obs_bits=True) == "step_observe_bits"
        assert env.rollout_actions_plan(slots) == "step_observe"
        tape = torch.from_numpy(make_tape(T, case["B"], case["n"], seed)).to(env.device)
        k = T if slots else 1
        buf = bits_buffers(env, k + 1)           # one slot more than the call may write: it stays 0xFFFFFFFF
        view = {"obs": buf["obs"][:k], "vec": buf["vec"][:k], "out": {key: v[:k] for key, v in buf["out"].items()}}
        env.rollout_actions(tape, slots=slots, obs_bits=True, **view)
        got = host(view["out"])
        for t in range(T):
            out, bits, vec = twin.step_observe_bits(tape[t])
            out = host(out)
            if slots or t == T - 1:
                q = t if slots else 0
                for key in out:
                    assert np.array_equal(got[key][q], out[key]), f"t={t}: {key}"
                assert torch.equal(buf["obs"][q], bits), f"t={t}: bits"
                assert torch.equal(buf["vec"][q].view(torch.int32), vec.view(torch.int32)), f"t={t}: vec"
        assert bool((buf["obs"][k] == -1).all()), "the slot after the last was written"
        sa, sb = env.get_state(), twin.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 6. band flag, launcher, capture
def test_band_clean_is_ignored_in_a_packed_launch():
    from mapf_amd import _lib
    from mapf_amd.env import _ptr, _stream
    name, T = "g_n8_20x20_f11", 23
    form = dict(roll_occ=4, roll_group=1)
    a, case, _, _, seed = case_env(name, form)
    b = case_env(name, form)[0]
    try:
        assert a.rollout_kernel_name(True, obs_bits=True) == "rollout_random_kernel<true,4,bits>"
        fa, fb = bits_buffers(a, T), bits_buffers(b, T)
        acts = [torch.full((T, e.B, e.N), -9, dtype=torch.int32, device=e.device) for e in (a, b)]
        flags = _lib.SLOTS | _lib.SLOTS_BAND_CLEAN | _lib.SLOTS_OBS_BITS
        so = a._make_stepout(fa["out"])
        _lib.check(_lib.lib().mapf_rollout_random(a.h, T, flags, _ptr(acts[0]), ctypes.byref(so), _ptr(fa["obs"]),
                                                  _ptr(fa["vec"]), _stream(a.device)))
        b.rollout_random(T, slots=True, actions=acts[1], obs_bits=True, **fb)
        torch.cuda.synchronize()
        assert torch.equal(fa["obs"], fb["obs"]) and not bool((fa["obs"] == -1).all(dim=-1).any())
        assert torch.equal(fa["vec"].view(torch.int32), fb["vec"].view(torch.int32))
        for key in fa["out"]:
            assert torch.equal(fa["out"][key], fb["out"][key]), key
    finally:
        a.close()
        b.close()


def test_packed_launcher_twice_equals_two_direct_calls():
    name, T = "g_n8_20x20_f11", 23
    a, case, _, _, seed = case_env(name)
    b = case_env(name)[0]
    try:
        fa = bits_buffers(a, T)
        acts = [torch.full((T, e.B, e.N), -9, dtype=torch.int32, device=e.device) for e in (a, b)]
        launch = a.rollout_launcher(T, slots=True, actions=acts[0], obs=fa["obs"], vec=fa["vec"], out=fa["out"], obs_bits=True)
        for call in range(2):
            fa["obs"].fill_(-1)
            launch()
            fb = bits_buffers(b, T)
            b.rollout_random(T, slots=True, actions=acts[1], obs_bits=True, **fb)
            torch.cuda.synchronize()
            assert torch.equal(fa["obs"], fb["obs"]), f"call {call}: bits"
            assert torch.equal(fa["vec"].view(torch.int32), fb["vec"].view(torch.int32)), f"call {call}: vec"
            assert torch.equal(acts[0], acts[1]), f"call {call}: actions"
            for key in fb["out"]:
                assert torch.equal(fa["out"][key], fb["out"][key]), f"call {call}: {key}"
        with pytest.raises(TypeError):
            a.rollout_launcher(T, slots=True, actions=acts[0], **slot_buffers(a, T), obs_bits=True)   # a float obs buffer
    finally:
        a.close()
        b.close()


def test_captured_packed_rollout_continues_the_episode():
    """One packed rollout_actions launch of the c4 shape (the three-wave form) captured and replayed
    twice over a refilled tape: 2T steps of the episode, every slot against the oracle."""
    name, T = "c4_40x40_n16_f9_looping", 12
    tape_h, ref, state = oracle_run(name, int(np.sum(LAUNCHES[:3])))
    env, case, _, _, _ = case_env(name)
    g = None
    try:
        assert env.rollout_actions_kernel_name(True, obs_bits=True).startswith("rollout_wide3_kernel<")
        buf = bits_buffers(env, T)
        tape = torch.from_numpy(tape_h[:T]).to(env.device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                env.rollout_actions(tape, slots=True, obs_bits=True, **buf)       # recorded, not run
        torch.cuda.synchronize()
        for call in range(2):
            tape.copy_(torch.from_numpy(tape_h[call * T:(call + 1) * T]))
            buf["obs"].fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            check_packed(f"replay {call}", env, ref, call * T, host(buf["out"]), buf["obs"], buf["vec"], [(q, q) for q in range(T)])
        check_state(env, state[2 * T], "after two replays")
        assert_no_errors(env, allow=(1, 2))
    finally:
        del g
        env.close()


# ------------------------------------------------------------------ 7. consumers
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n,C,F", [(1, 5, 1), (3, 6, 7), (37, 6, 11), (5, 7, 11), (130, 6, 9)])
def test_unpack_obs_kernel(n, C, F, dtype):
    """mapf_unpack_obs into a destination that starts 4 bytes into its storage (4-byte alignment only;
    C*F*F is odd at (5, 1), (6, 7)... and no multiple of 4 at c2 / c5), guard elements on both sides."""
    from mapf_amd.env import unpack_obs
    rng = np.random.default_rng([n, C, F])
    obs = (rng.random((n, C, F, F)) < 0.3).astype(np.float32)
    bits = torch.from_numpy(pack_np(obs, C, F).view(np.int32).copy()).cuda()
    cff, lead = n * C * F * F, 4 // torch.empty((), dtype=dtype).element_size()
    store = torch.full((lead + cff + 8,), 7.0, dtype=dtype, device="cuda")
    dst = store[lead:lead + cff].view(n, C, F, F)
    assert dst.data_ptr() % 16 == 4
    assert unpack_obs(bits, C, F, dtype=dtype, out=dst) is dst
    torch.cuda.synchronize()
    assert np.array_equal(dst.float().cpu().numpy(), obs)
    assert bool((store[:lead] == 7).all()) and bool((store[lead + cff:] == 7).all()), "wrote outside dst"
    assert np.array_equal(unpack_obs(bits, C, F, dtype=dtype).float().cpu().numpy(), obs)


def test_unpack_obs_of_no_agents_launches_nothing():
    from mapf_amd import _lib
    from mapf_amd.env import unpack_obs
    out = unpack_obs(torch.empty(0, 16, dtype=torch.int32, device="cuda"), 6, 9)
    assert tuple(out.shape) == (0, 6, 9, 9)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert _lib.lib().mapf_unpack_obs(None, None, 0, 6, 9, 0, ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert tape_tests.graph_shape(g.raw_cuda_graph())[:2] == (0, 0)
    assert _lib.lib().mapf_unpack_obs(None, None, 1, 6, 9, 0, None) != 0
    del g


@pytest.mark.parametrize("nimg,C,F", [(37, 6, 9), (5, 7, 11), (1, 6, 9)])
def test_conv_first_bits_is_conv_first_f32_bit_for_bit(nimg, C, F):
    """mapf_conv_first_bits on the packed input == mapf_conv_first_f32 on the unpacked floats (37
    images of 81 pixels: 2,997 pixels, ragged against the 128-pixel tile)."""
    from mapf_amd import _lib
    rng = np.random.default_rng([nimg, C, F])
    obs = (rng.random((nimg, C, F, F)) < 0.3).astype(np.float32)
    x = torch.from_numpy(obs).cuda()
    bits = torch.from_numpy(pack_np(obs, C, F).view(np.int32).copy()).cuda()
    g = torch.Generator().manual_seed(nimg)
    w = torch.zeros(128, 64, dtype=torch.float16)
    w[:, :C * 9] = (torch.randn(128, C * 9, generator=g) * 0.2).half()
    w, b = w.cuda(), (torch.randn(128, generator=g) * 0.1).half().cuda()
    y = [torch.full((nimg, F, F, 128), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2)]
    _lib.call("mapf_conv_first_f32", x, w, b, y[0], nimg, C, F, F, 128)
    _lib.call("mapf_conv_first_bits", bits, w, b, y[1], nimg, C, F, F, 128)
    torch.cuda.synchronize()
    assert torch.equal(y[0].view(torch.int16), y[1].view(torch.int16))
    assert bool(torch.isfinite(y[0].float()).all()) and bool((y[0] > 0).any())
