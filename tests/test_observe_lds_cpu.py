"""CPU checks of the mapf_observe launch's LDS request and of how the envs per observe workgroup are
fitted to a device's limit (include/mapf.h: mapf_observe_lds, mapf_tuning.obs_envs) -- the host side
of observe_lds / observe_fit_envs (csrc/mapf_observe.hip), the functions launch_observe, mapf_create
and mapf_set_tuning run.  libmapf.so loads without a GPU.

The default rule (64 / N envs per workgroup for N <= 8) ignores the map: every env brings an H*W-byte
agent-index image, so few agents on a large map asked for several times the LDS a workgroup can
have.  Both limits a gfx950 runtime may report are covered: 64 KiB and 160 KiB."""
import ctypes
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMITS = (65536, 163840)
K_PREDICT = 5      # make_config: TrainingParameters.K_TIMESTEP_PREDICT


def config(N, H, W, F, C, shared, B, keep_bfs=True, k_predict=None):
    """k_predict None: make_config's own value, which must be K_PREDICT (what regions() assumes by default)."""
    from mapf_amd.config import make_config
    cfg = make_config(B, H, W, num_agents=N, fov=F, num_channel=C, shared_map=shared, keep_bfs=keep_bfs,
                      k_predict=k_predict)
    assert cfg.k_predict == (K_PREDICT if k_predict is None else k_predict)
    return cfg


def observe_lds(cfg, obs_envs, max_lds):
    """(bytes or negative error, envs_out)"""
    from mapf_amd import _lib
    envs = ctypes.c_int32(-77)
    got = _lib.lib().mapf_observe_lds(ctypes.byref(cfg), obs_envs, max_lds, ctypes.byref(envs))
    return int(got), int(envs.value)


def rule(N, B):
    return min(64 // N if N <= 8 else 1, B)


def regions(N, H, W, F, C, shared, keep_bfs, E, K=K_PREDICT):
    """The observing workgroup's LDS, region by region (csrc/mapf_observe.h: obs_lds_bytes /
    obs_layout; the nibble table: observe_kernel), in bytes."""
    P = max(F // 2, 1)
    rowsz = (H + 2 * P) * ((W + 2 * P + 31) // 32)              # padded obstacle rows of one map, in words
    r = dict(
        stream=4 * (((E * N * C * F * F + 31) // 32 + 1 + 3) & ~3),   # one bit per float + a spare word, 4-word units
        occupancy=4 * E * rowsz,
        maps=4 * (1 if shared else E) * rowsz,
        agents=4 * (2 * E * N + E),                             # every agent's cell and goal, each env's human next cell
        prediction=4 * (E * K + E),                             # human.path[1..K] and its count
        bfs_windows=4 * E * N * (F * ((F + 2) >> 1) + 1) if C >= 7 and keep_bfs and W % 2 == 0 else 0,
        index_image=(E * H * W + 3) & ~3)
    body = sum(r.values())
    r["round_up"] = -body % 16
    r["nibble_table"] = 256
    return r


def search_lds(H, W):
    """LDS of the four search waves an observe launch hosts on narrow maps (csrc/mapf_search.h: wave_lds)."""
    if W > 32 or H > 64:
        return 0
    return 4 * ((max(3 * 64 * 4, ((H * W + 7) & ~7) * 2) + 15) & ~15)


def request(N, H, W, F, C, shared, keep_bfs, E, K=K_PREDICT):
    return max(sum(regions(N, H, W, F, C, shared, keep_bfs, E, K).values()), search_lds(H, W))


SIZES = [(s, s) for s in (10, 20, 40, 64, 80, 128)] + [(64, 32)]
ODD_W = [(21, 21), (80, 79)]          # C = 7: obs_bfs_windows is off at odd W (the BFS channel straight from HBM)


def grid():
    for N, F, shared, B in itertools.product((1, 2, 3, 4, 7, 8, 9, 16, 64), (3, 7, 9, 11, 16), (True, False),
                                             (1, 37, 4096)):
        for C in (5, 6, 7):
            for H, W in SIZES + (ODD_W if C == 7 else []):
                yield N, H, W, F, C, shared, B


def test_fitted_envs_over_the_grid():
    """Every point, both limits: the fitted count is within 1..min(rule, B), its request fits, it is the
    rule wherever the rule's own request fits, and it is maximal.  The request of every count asked
    about equals the plain sum of regions().

    One env of the largest configurations (e.g. 64 agents on 128x128 at FOV 16 with the BFS windows:
    74 KB) does not fit 64 KiB at all: there no count can be right, and the call must say so -- 0 envs
    and MAPF_EINVAL, what mapf_create answers -- which is asserted in place of the four properties, only
    where the plain sum for ONE env is over the limit.  Under 160 KiB every point fits."""
    npoints = reduced = nofit = 0
    for N, H, W, F, C, shared, B in grid():
        cfg = config(N, H, W, F, C, shared, B)
        r = rule(N, B)
        unfitted, e0 = observe_lds(cfg, 0, 0)
        assert (unfitted, e0) == (request(N, H, W, F, C, shared, True, r), r), (N, H, W, F, C, shared, B)
        for limit in LIMITS:
            point = (N, H, W, F, C, shared, B, limit)
            got, envs = observe_lds(cfg, 0, limit)
            npoints += 1
            if request(N, H, W, F, C, shared, True, 1) > limit:
                assert limit == 65536 and (got, envs) == (-1, 0), point
                nofit += 1
                continue
            assert 1 <= envs <= r, point
            assert 0 < got <= limit, point
            assert got == request(N, H, W, F, C, shared, True, envs), point
            if unfitted <= limit:
                assert envs == r and got == unfitted, point
            else:
                assert envs < r, point
                reduced += 1
            if envs < r:                                        # maximal: one more env does not fit
                more, e1 = observe_lds(cfg, envs + 1, 0)
                assert e1 == envs + 1 and more > limit, point
            # an explicit value goes through the same fit
            assert observe_lds(cfg, r, limit) == (got, envs), point
    assert npoints == 2 * (9 * 5 * 2 * 3) * (3 * 7 + 2) and reduced > 500 and 0 < nofit < npoints // 20


def test_presets_keep_their_default():
    """bench.PRESETS launch what they launched before the fit: 16 / 8 / 1 / 1 envs per workgroup for
    c1 / c2 / c4 / c5 (c1 at its own single env: 1), at either limit."""
    import bench
    want = dict(c1=16, c2=8, c4=1, c5=1)
    assert set(bench.PRESETS) == set(want)
    for name, p in bench.PRESETS.items():
        shared = p["maps"] == "warehouse"                       # bench.make_maps
        for B in (p["envs"], 4096):
            cfg = config(p["agents"], p["size"], p["size"], p["fov"], p["channels"], shared, B)
            unfitted, e0 = observe_lds(cfg, 0, 0)
            assert e0 == min(want[name], B) == rule(p["agents"], B)
            for limit in LIMITS:
                assert observe_lds(cfg, 0, limit) == (unfitted, e0), (name, B, limit)


# (N, H, W, F, C, shared, keep_bfs, E)
BYTE_POINTS = [
    (8, 20, 20, 11, 6, True, True, 8),        # c2: 11,104 B
    (8, 20, 20, 11, 6, True, True, 64),       # ... and an explicit obs_envs = 64 there: ~80 KB
    (4, 10, 10, 11, 6, True, True, 16),       # c1
    (16, 40, 40, 9, 6, True, True, 1),        # c4
    (64, 80, 80, 11, 7, False, True, 1),      # c5: BFS windows
    (64, 80, 79, 11, 7, False, True, 1),      # odd W: no windows, index image rounded up to 4
    (1, 80, 80, 11, 6, False, True, 64),      # the named shapes
    (2, 80, 80, 9, 6, True, True, 32),
    (1, 64, 64, 7, 6, False, True, 64),
    (3, 21, 21, 3, 5, False, False, 5),       # FOV 3: padding 1; odd everything
    (7, 64, 32, 16, 7, True, True, 9),        # even FOV, a hosted search of 4 * 4096 B below the request
    (9, 128, 128, 16, 7, False, True, 2),
    (1, 10, 10, 3, 5, True, False, 1),        # the smallest: 512 B, so the hosted search's 4 * 768 B is the request
    (1, 64, 32, 3, 5, True, False, 1),        # ... and the largest hosted search, 4 * 4096 B
]


def test_request_is_the_sum_of_its_regions():
    """The layout arithmetic the kernels index by, at a dozen points: bit-stream, occupancy, map
    copies, agent words, prediction slots, BFS windows, index image, the 16-byte round-up and the
    256-byte nibble table -- or the hosted search's four waves where that is more."""
    hosted = 0
    for N, H, W, F, C, shared, keep_bfs, E in BYTE_POINTS:
        cfg = config(N, H, W, F, C, shared, 4096, keep_bfs=keep_bfs)
        r = regions(N, H, W, F, C, shared, keep_bfs, E)
        own = sum(r.values())
        assert own % 16 == 0 and 0 <= r["round_up"] < 16
        assert (r["bfs_windows"] > 0) == (C == 7 and W % 2 == 0)
        want = max(own, search_lds(H, W))
        hosted += want > own
        assert observe_lds(cfg, E, 0) == (want, E), (N, H, W, F, C, shared, keep_bfs, E)
    assert hosted == 2
    assert observe_lds(config(1, 10, 10, 3, 5, True, 4096, keep_bfs=False), 1, 0)[0] == 4 * 768
    assert observe_lds(config(1, 64, 32, 3, 5, True, 4096, keep_bfs=False), 1, 0)[0] == 4 * 4096
    # hand-computed anchors, so that regions() itself cannot drift with the library.  c2, 8 envs:
    # stream 5,824 + occupancy 960 + map 120 + agents 544 + prediction 192 + image 3,200 = 10,840 -> 10,848 + 256
    assert sum(regions(8, 20, 20, 11, 6, True, True, 8).values()) == 11104
    assert regions(1, 80, 80, 11, 6, False, True, 64)["index_image"] == 409600


@pytest.mark.parametrize("K", [0, 1, 64])
def test_request_follows_k_predict(K):
    """The prediction rows are E * k_predict words (+ E counts): at K = 0 the region is the counts alone,
    and the request at every byte point equals the plain sum with that K -- 4 * E * (K - 5) bytes from the
    default's, before the 16-byte round-up."""
    for N, H, W, F, C, shared, keep_bfs, E in BYTE_POINTS:
        cfg = config(N, H, W, F, C, shared, 4096, keep_bfs=keep_bfs, k_predict=K)
        r = regions(N, H, W, F, C, shared, keep_bfs, E, K=K)
        assert r["prediction"] == 4 * E * (K + 1)
        base = regions(N, H, W, F, C, shared, keep_bfs, E)
        assert sum(r.values()) - r["round_up"] == sum(base.values()) - base["round_up"] + 4 * E * (K - K_PREDICT)
        want = request(N, H, W, F, C, shared, keep_bfs, E, K)
        assert observe_lds(cfg, E, 0) == (want, E), (K, N, H, W, F, C, shared, keep_bfs, E)
    # c2, 8 envs, by hand: 11,104 B at K = 5 is 10,840 + 8 + 256; K = 64 adds 8 * 59 * 4 = 1,888 -> 12,728 -> 12,736 + 256
    assert observe_lds(config(8, 20, 20, 11, 6, True, 4096, k_predict=64), 8, 0)[0] == 12992
    assert observe_lds(config(8, 20, 20, 11, 6, True, 4096, k_predict=0), 8, 0)[0] == 10688 + 256


NAMED = [(1, 80, 80, 11, False, 64), (2, 80, 80, 9, True, 32), (1, 64, 64, 7, False, 64)]


@pytest.mark.parametrize("N,H,W,F,shared,B", NAMED)
def test_named_shapes_exceed_the_limit_unfitted_and_fit_fitted(N, H, W, F, shared, B):
    cfg = config(N, H, W, F, 6, shared, B)
    unfitted, e0 = observe_lds(cfg, 0, 0)
    assert e0 == 64 // N == B and unfitted > 163840
    for limit in LIMITS:
        got, envs = observe_lds(cfg, 0, limit)
        assert 1 <= envs < e0 and 0 < got <= limit
        assert observe_lds(cfg, envs + 1, 0)[0] > limit


def test_bad_arguments_are_rejected():
    from mapf_amd import _lib
    L = _lib.lib()
    cfg = config(8, 20, 20, 11, 6, True, 64)
    assert L.mapf_observe_lds(None, 0, 0, None) == -1
    assert L.mapf_observe_lds(ctypes.byref(cfg), 65, 0, None) == -1 and b"obs_envs" in L.mapf_last_error()
    assert L.mapf_observe_lds(ctypes.byref(cfg), -1, 0, None) == -1
    assert L.mapf_observe_lds(ctypes.byref(cfg), 0, -1, None) == -1
    assert L.mapf_observe_lds(ctypes.byref(cfg), 8, 65536, None) == 11104       # envs_out may be NULL
    # an explicit 64 at c2's shape: 80 KB, over 64 KiB (the fit names what mapf_set_tuning's message does)
    big = request(8, 20, 20, 11, 6, True, True, 64)
    assert 65536 < big <= 163840 and observe_lds(cfg, 64, 0) == (big, 64) and observe_lds(cfg, 64, 163840) == (big, 64)
    got, envs = observe_lds(cfg, 64, 65536)
    assert 8 <= envs < 64 and got == request(8, 20, 20, 11, 6, True, True, envs) <= 65536
    assert request(8, 20, 20, 11, 6, True, True, envs + 1) > 65536
    bad = config(65, 20, 20, 11, 6, True, 64)                                   # mapf_create's own checks
    assert L.mapf_observe_lds(ctypes.byref(bad), 0, 0, None) == -1 and b"num_agents" in L.mapf_last_error()
    tiny = config(64, 128, 128, 16, 7, False, 4)                                # one env: 74 KB
    assert observe_lds(tiny, 0, 65536) == (-1, 0) and b"LDS" in L.mapf_last_error()
    assert observe_lds(tiny, 0, 163840)[1] == 1
