"""CPU checks of the grid symmetries (include/mapf.h: "Grid symmetries"): the host twins run the
__host__ __device__ functions of csrc/mapf_sym.h that the gather and draw kernels run, so the group
law, the equivariance of the env (against the oracle) and the draws are settled here without a GPU."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

GS = range(8)


def L():
    from mapf_amd import _lib
    return _lib.lib()


def np_plane(x, g):
    """the definition: an optional column mirror, then g & 3 counter-clockwise quarter turns"""
    return np.ascontiguousarray(np.rot90(np.flip(x, -1) if g & 4 else x, k=g & 3, axes=(-2, -1)))


def sym_obs(obs, g):
    obs = np.ascontiguousarray(obs, np.float32)
    C, F = obs.shape[-3], obs.shape[-1]
    out = np.full_like(obs, -9)
    assert L().mapf_sym_obs_host(obs.ctypes.data, obs.size // (C * F * F), C, F, g, out.ctypes.data) == 0
    return out


def sym_vec(vec, g):
    vec = np.ascontiguousarray(vec, np.float32)
    out = np.full_like(vec, -9)
    assert L().mapf_sym_vec_host(vec.ctypes.data, vec.size // 4, g, out.ctypes.data) == 0
    return out


def sym_cols(cols, g):
    cols = np.ascontiguousarray(cols, np.float32)
    out = np.full_like(cols, -9)
    assert L().mapf_sym_cols_host(cols.ctypes.data, cols.size // 5, g, out.ctypes.data) == 0
    return out


def sym_actions(a, g):
    return np.array([L().mapf_sym_action(g, int(x)) for x in np.asarray(a).reshape(-1)], np.int64).reshape(np.shape(a))


def sym_cell(g, F, r, c):
    r2, c2 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L().mapf_sym_cell(g, F, r, c, ctypes.byref(r2), ctypes.byref(c2)) == 0
    return r2.value, c2.value


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ T1: the group law
@pytest.mark.parametrize("F", [1, 3, 9, 11])
@pytest.mark.parametrize("C", [5, 6, 7])
def test_obs_host_is_the_numpy_expression(C, F):
    rng = np.random.default_rng(C * 100 + F)
    obs = (rng.random((3, C, F, F)) < 0.4).astype(np.float32)
    for g in GS:
        np.testing.assert_array_equal(sym_obs(obs, g), np_plane(obs, g), err_msg=f"g={g}")


@pytest.mark.parametrize("F", [1, 3, 9])
def test_cell_agrees_with_the_plane_map(F):
    for g in GS:
        for r in range(F):
            for c in range(F):
                x = np.zeros((F, F), np.float32)
                x[r, c] = 1
                r2, c2 = sym_cell(g, F, r, c)
                assert np_plane(x, g)[r2, c2] == 1, (g, r, c)


def test_compose_and_inverse_agree_with_numpy():
    x = np.arange(25, dtype=np.float32).reshape(5, 5)          # no symmetry of its own: the planes name g
    planes = [np_plane(x, g) for g in GS]
    which = lambda y: next(g for g in GS if np.array_equal(planes[g], y))   # noqa: E731
    for g1 in GS:
        assert which(np_plane(np_plane(x, g1), L().mapf_sym_inverse(g1))) == 0
        for g2 in GS:
            assert L().mapf_sym_compose(g1, g2) == which(np_plane(np_plane(x, g1), g2)), (g1, g2)


def test_actions_vec_and_columns_are_homomorphisms():
    rng = np.random.default_rng(5)
    vec = rng.standard_normal((6, 4)).astype(np.float32)
    vec[0, 0] = vec[1, 1] = 0.0
    vec[2, :2] = 0.0
    cols = rng.random((6, 5)).astype(np.float32)
    acts = np.array([0, 1, 2, 3, 4, 7, -1, 5])
    # the tables of the issue: a quarter turn and the mirror
    np.testing.assert_array_equal(sym_actions(acts, 1), [0, 4, 1, 2, 3, 7, -1, 5])
    np.testing.assert_array_equal(sym_actions(acts, 4), [0, 3, 2, 1, 4, 7, -1, 5])
    np.testing.assert_array_equal(bits(sym_vec(vec, 1)), bits(np.stack([0.0 - vec[:, 1], vec[:, 0], vec[:, 2], vec[:, 3]], 1)))
    np.testing.assert_array_equal(bits(sym_vec(vec, 4)), bits(np.stack([vec[:, 0], 0.0 - vec[:, 1], vec[:, 2], vec[:, 3]], 1)))
    for g1 in GS:
        for g2 in GS:
            g12 = L().mapf_sym_compose(g1, g2)
            np.testing.assert_array_equal(sym_actions(sym_actions(acts, g1), g2), sym_actions(acts, g12))
            np.testing.assert_array_equal(bits(sym_vec(sym_vec(vec, g1), g2)), bits(sym_vec(vec, g12)))
            np.testing.assert_array_equal(bits(sym_cols(sym_cols(cols, g1), g2)), bits(sym_cols(cols, g12)))
        # the columns move with the actions
        for a in range(5):
            np.testing.assert_array_equal(sym_cols(cols, g1)[:, L().mapf_sym_action(g1, a)], cols[:, a])


@pytest.mark.parametrize("F", [1, 3, 9])
def test_inverse_restores_every_array_bit_for_bit(F):
    rng = np.random.default_rng(F)
    obs = (rng.random((3, 6, F, F)) < 0.5).astype(np.float32)
    vec = rng.standard_normal((5, 4)).astype(np.float32)
    vec[0, :2] = 0.0                                            # +0.0 stays +0.0 through g and back
    vec[1, 1] = 0.0
    cols = rng.random((5, 5)).astype(np.float32)
    acts = np.array([0, 1, 2, 3, 4, 9])
    for g in GS:
        gi = L().mapf_sym_inverse(g)
        np.testing.assert_array_equal(bits(sym_obs(sym_obs(obs, g), gi)), bits(obs))
        np.testing.assert_array_equal(bits(sym_vec(sym_vec(vec, g), gi)), bits(vec))
        np.testing.assert_array_equal(bits(sym_cols(sym_cols(cols, g), gi)), bits(cols))
        np.testing.assert_array_equal(sym_actions(sym_actions(acts, g), gi), acts)
        out = sym_vec(vec, g)
        assert (out == 0).sum() == (vec == 0).sum() and not np.signbit(out[out == 0]).any(), g


# ------------------------------------------------------------------ T2: equivariance against the oracle
SCENE_H, SCENE_W, SCENE_F, SCENE_C, SCENE_N = 7, 9, 5, 7, 3
SCENE_OBSTACLES = [(0, 3), (2, 4), (4, 2), (5, 6), (6, 0), (1, 7)]
SCENE_AGENTS = [((1, 1), (5, 7)), ((1, 2), (0, 8)), ((4, 4), (2, 6))]      # (start, goal); 0 and 1 side by side
SCENE_HUMAN = ((3, 0), (3, 8))              # one row, only free cells between: the shortest path is unique


def grid_cell(g, H, W, r, c):
    """mapf_sym_cell's rule on an H x W grid: mirror (r, W-1-c); quarter turn (r, c) -> (W-1-c, r), H x W -> W x H"""
    if g & 4:
        c = W - 1 - c
    for _ in range(g & 3):
        r, c, H, W = W - 1 - c, r, W, H
    return r, c


def scene(g=0):
    """The scene transformed by g: (oracle config, world, agent sequences, human start, human goal)."""
    H, W = SCENE_H, SCENE_W
    world = np.zeros((H, W), np.int8)
    for r, c in SCENE_OBSTACLES:
        world[r, c] = -1
    w2 = np_plane(world, g)
    tr = lambda p: grid_cell(g, H, W, *p)       # noqa: E731
    cfg = O.make_config(w2.shape[0], w2.shape[1], SCENE_N, SCENE_F, SCENE_C, use_da=1, use_hp=1, human_mode=0,
                        goal_mode=0, fix_choice=0, keep_bfs=1, max_seq=2, seed=11, k_predict=3, penalty_radius=2)
    seqs = [[tr(s), tr(t)] for s, t in SCENE_AGENTS]
    return cfg, w2, seqs, tr(SCENE_HUMAN[0]), tr(SCENE_HUMAN[1])


def scene_env(g=0):
    cfg, world, seqs, hs, hg = scene(g)
    oe = O.OracleEnv(cfg)
    assert oe.reset_fixed(world, seqs, hs, hg) == 0
    return oe


def test_grid_cell_extends_sym_cell():
    for g in GS:
        for r in range(5):
            for c in range(5):
                assert grid_cell(g, 5, 5, r, c) == sym_cell(g, 5, r, c)
        x = np.zeros((SCENE_H, SCENE_W), np.int8)
        x[2, 7] = 1
        assert np_plane(x, g)[grid_cell(g, SCENE_H, SCENE_W, 2, 7)] == 1


@pytest.mark.parametrize("g", GS)
def test_oracle_env_is_equivariant(g):
    base, other = scene_env(0), scene_env(g)
    # the scene's human path is unique: the transformed env walks the transform of the original's path
    path = base.human_path()
    assert len(path) >= SCENE_W
    want_path = np.array([grid_cell(g, SCENE_H, SCENE_W, r, c) for r, c in path], np.int32)
    np.testing.assert_array_equal(other.human_path(), want_path)
    obs, vec = base.observe()
    assert all(obs[:, ch].any() for ch in range(SCENE_C)), "every channel of the scene is exercised"
    obs2, vec2 = other.observe()
    np.testing.assert_array_equal(bits(obs2), bits(sym_obs(obs, g)))
    np.testing.assert_array_equal(bits(vec2), bits(sym_vec(vec, g)))
    # train_valid of one step under transformed actions = the columns map of the original's
    seen, stepped = set(), 0
    for acts in ([1, 3, 0], [2, 2, 4], [0, 0, 0], [3, 1, 2], [4, 3, 1]):
        a, b = scene_env(0), scene_env(g)
        ra = a.step(np.array(acts, np.int32))
        va = ra["valid"]
        vb = b.step(sym_actions(acts, g).astype(np.int32))["valid"]
        np.testing.assert_array_equal(vb, sym_cols(va, g), err_msg=f"actions {acts}")
        seen |= set(np.unique(va).tolist())
        if not (ra["status"] > 0).all():
            continue            # fixActions repairs a collision in agent order: not a symmetric rule
        stepped += 1
        # a step that needs no repair commutes with g, the human's move included
        oa, wa = a.observe()
        ob, wb = b.observe()
        np.testing.assert_array_equal(bits(ob), bits(sym_obs(oa, g)), err_msg=f"after actions {acts}")
        np.testing.assert_array_equal(bits(wb), bits(sym_vec(wa, g)))
    assert seen == {0.0, 1.0} and stepped >= 2


# ------------------------------------------------------------------ T3: the draws
def host_draw(seed, epoch, start, count, allowed):
    buf = np.full(count + 2, 99, np.uint8)
    rc = L().mapf_sym_draw_host(seed, epoch, start, count, allowed, buf.ctypes.data)
    assert rc == 0, L().mapf_last_error()
    assert (buf[count:] == 99).all()
    return buf[:count].copy()


@pytest.mark.parametrize("allowed", [0xFF, 0x0F, 0x01, 0xA5, 0x80, 0x30])
def test_draws_respect_allowed_and_hit_every_element(allowed):
    d = host_draw(7, 3, 0, 4096, allowed)
    assert set(d.tolist()) == {g for g in GS if allowed >> g & 1}


def test_draws_are_uniform_enough():
    counts = np.bincount(host_draw(1, 0, 0, 4096, 0xFF), minlength=8)
    # 4,096 draws over 8 values: mean 512, sigma 21.2; six sigma either side
    assert counts.min() > 512 - 128 and counts.max() < 512 + 128, counts


def test_a_window_is_a_slice_of_a_longer_window():
    full = host_draw(2 ** 63 + 9, 5, 100, 1000, 0xFF)
    np.testing.assert_array_equal(host_draw(2 ** 63 + 9, 5, 350, 200, 0xFF), full[250:450])
    big = 2 ** 32 - 8                                           # across the counter's low word
    np.testing.assert_array_equal(host_draw(1, 1, big + 4, 8, 0x0F), host_draw(1, 1, big, 16, 0x0F)[4:12])
    assert not np.array_equal(host_draw(1, 1, 0, 64, 0xFF), host_draw(1, 2, 0, 64, 0xFF))
    assert not np.array_equal(host_draw(1, 1, 0, 64, 0xFF), host_draw(2, 1, 0, 64, 0xFF))


def test_draw_is_the_specified_philox_pick():
    d = host_draw(0x1234, 6, 40, 16, 0xB6)
    members = [g for g in GS if 0xB6 >> g & 1]
    for j in range(16):
        word = O.philox_word(40 + j, 13, 6, 0, 0x1234, 0)
        assert d[j] == members[(word * len(members)) >> 32]


def test_draw_refusals_and_wrapper():
    import torch
    from mapf_amd.env import sym_draw
    buf = np.zeros(4, np.uint8)
    assert L().mapf_sym_draw_host(0, 0, 0, 4, 0, buf.ctypes.data) == -1 and b"allowed" in L().mapf_last_error()
    assert L().mapf_sym_draw(0, 0, 0, 4, 0, buf.ctypes.data, None) == -1        # refused before any device call
    assert L().mapf_sym_draw_host(0, 0, -1, 4, 1, buf.ctypes.data) == -1
    assert L().mapf_sym_draw_host(0, 0, 0, 4, 1, None) == -1
    got = sym_draw(7, 3, 10, 50, 0x0F, device="cpu")
    assert got.dtype == torch.uint8 and got.device.type == "cpu"
    np.testing.assert_array_equal(got.numpy(), host_draw(7, 3, 10, 50, 0x0F))
    with pytest.raises(RuntimeError, match="allowed"):
        sym_draw(7, 3, 10, 50, 0, device="cpu")


# ------------------------------------------------------------------ T4: refusals, and sym_apply
def gather_spec(kind=1, N=2, C=6, F=3, src_bytes=None, dst_bytes=None, sym=True, dst=True):
    from mapf_amd import _lib
    row = N * C * F * F * 4
    spec = _lib.GatherSymSpec(T=2, B=3, M=4, rows=64, sym=128 if sym else None, N=N, C=C, F=F, count=1)
    spec.arrays[0] = _lib.GatherSymArray(256, 512 if dst else None, row if src_bytes is None else src_bytes,
                                         row if dst_bytes is None else dst_bytes, kind, 0)
    return spec


@pytest.mark.parametrize("spec, field", [
    (dict(F=4), b"F"), (dict(F=17, sym=False), b"F"), (dict(F=0, sym=False), b"F"), (dict(C=8), b"C"), (dict(C=0), b"C"),
    (dict(kind=7), b"kind"), (dict(kind=-1), b"kind"),
    (dict(src_bytes=2 * 6 * 9 * 4 + 4), b"row_bytes"), (dict(dst_bytes=2 * 6 * 9 * 4 - 4), b"row_bytes"),
    (dict(kind=2), b"row_bytes"),                 # a packed source has N * WPA words, not N * C * F * F
    (dict(kind=3), b"row_bytes"), (dict(kind=6), b"row_bytes"), (dict(kind=0, dst_bytes=8), b"row_bytes"),
    (dict(dst=False), b"dst"), (dict(N=0), b"N"),
])
def test_gather_rows_sym_refuses_before_any_launch(spec, field):
    """the pointers are made up: a spec that got past the checks would fault, a refused one touches nothing"""
    s = gather_spec(**spec)
    assert L().mapf_gather_rows_sym(ctypes.byref(s), None) == -1
    assert field in L().mapf_last_error(), L().mapf_last_error()


def test_gather_rows_sym_refuses_null_spec_and_rows():
    assert L().mapf_gather_rows_sym(None, None) == -1
    s = gather_spec()
    s.rows = None
    assert L().mapf_gather_rows_sym(ctypes.byref(s), None) == -1 and b"null" in L().mapf_last_error()
    s = gather_spec()
    s.count = 17
    assert L().mapf_gather_rows_sym(ctypes.byref(s), None) == -1 and b"count" in L().mapf_last_error()


def test_sym_apply_equals_the_host_twins():
    import torch
    from mapf_amd.env import sym_apply
    rng = np.random.default_rng(3)
    M, N, C, F = 11, 3, 6, 5
    obs = (rng.random((M, N, C, F, F)) < 0.4).astype(np.float32)
    vec = rng.standard_normal((M, N, 4)).astype(np.float32)
    vec[0, :, :2] = 0.0
    acts = rng.integers(0, 6, (M, N))                          # 5 is out of range: copied
    cols = rng.random((M, N, 5)).astype(np.float32)
    g = np.array([0, 1, 2, 3, 4, 5, 6, 7, 3, 3, 6], np.uint8)
    want = ([sym_obs(obs[j], int(g[j])) for j in range(M)], [sym_vec(vec[j], int(g[j])) for j in range(M)],
            [sym_actions(acts[j], int(g[j])) for j in range(M)], [sym_cols(cols[j], int(g[j])) for j in range(M)])
    for dtype in (torch.int32, torch.int64):
        o, v, a, c = sym_apply(torch.from_numpy(obs), torch.from_numpy(vec), torch.from_numpy(acts).to(dtype),
                               torch.from_numpy(cols), torch.from_numpy(g))
        assert a.dtype == dtype
        np.testing.assert_array_equal(bits(o.numpy()), bits(np.stack(want[0])))
        np.testing.assert_array_equal(bits(v.numpy()), bits(np.stack(want[1])))
        np.testing.assert_array_equal(a.numpy(), np.stack(want[2]))
        np.testing.assert_array_equal(bits(c.numpy()), bits(np.stack(want[3])))
    # numpy in, numpy out; one g for every row; None passes through
    o, v, a, c = sym_apply(obs, None, acts, None, 5)
    assert isinstance(o, np.ndarray) and v is None and c is None
    np.testing.assert_array_equal(o, np.stack([sym_obs(obs[j], 5) for j in range(M)]))
    np.testing.assert_array_equal(a, sym_actions(acts, 5))
    with pytest.raises(ValueError):
        sym_apply(obs, None, None, None, [0, 1])


@pytest.mark.parametrize("packed", [False, True])
def test_imitate_rows_off_the_gpu_applies_sym_apply(packed):
    """a CPU model trains through imitation_train on torch-indexed rows: with sym= they are sym_apply's"""
    import types
    import torch
    from mapf_amd.env import pack_obs, sym_apply
    from mapf_amd.model import Model
    T_, B_, N, C, F = 2, 3, 8, 6, 9
    rng = np.random.default_rng(8)
    obs = torch.from_numpy((rng.random((T_ + 1, B_, N, C, F, F)) < 0.3).astype(np.float32))
    vec = torch.from_numpy(rng.standard_normal((T_ + 1, B_, N, 4)).astype(np.float32))
    act = torch.from_numpy(rng.integers(0, 5, (T_, B_, N))).int()
    source = types.SimpleNamespace(T=T_, env=types.SimpleNamespace(B=B_, C=C, F=F), packed=packed, vec=vec,
                                   expert_actions=act, obs=None if packed else obs,
                                   obs_bits=pack_obs(obs, C, F) if packed else None)
    model = Model(0, "cpu", global_model=True, numChannel=C, num_agents=N, fov=F)
    seen = []
    model.imitation_train = lambda o, v, a, s: seen.append((o, v, a)) or [0.0, 0.0]
    rows, sym = [5, 0, 3, 3], [6, 0, 1, 3]
    model.imitate_rows(source, rows, sym=sym)
    model.imitate_rows(source, rows)
    r = torch.tensor(rows)
    ts, bs = r % T_, r // T_
    want = sym_apply(obs[ts, bs], vec[ts, bs], act[ts, bs], None, sym)
    for got, w in zip(seen[0], want):
        assert torch.equal(got, w)
    assert torch.equal(seen[1][0], (source.obs_bits if packed else obs)[ts, bs]) and torch.equal(seen[1][2], act[ts, bs])
    with pytest.raises(ValueError):
        model.imitate_rows(source, rows, sym=[0.5, 0, 1, 3])
