"""CPU checks of the clean-band skip set (MAPF_SLOTS_BAND_CLEAN, include/mapf.h): the host side of
obs_band_skip (csrc/mapf_observe.h), the one function the rollout kernel runs too, exported as
mapf_obs_band_skip.  libmapf.so loads without a GPU."""
import ctypes

import numpy as np
import pytest

SHAPES = [(8, 6, 11), (6, 6, 9), (8, 6, 7)]          # (N, C, F)
UNITS = [16, 64, 128]
OFFSETS = list(range(0, 128, 16))


def skip_bitmap(N, C, F, unit, off, B=64, **kw):
    from mapf_amd import _lib
    from mapf_amd.config import make_config
    cfg = make_config(B, 20, 20, num_agents=N, fov=F, num_channel=C, **kw)
    nq = N * C * F * F // 4
    buf = np.full(nq + 8, 9, np.uint8)                 # the 8 past the end must stay untouched
    got = _lib.lib().mapf_obs_band_skip(ctypes.byref(cfg), unit, off, buf.ctypes.data, nq)
    assert got == nq, _lib.lib().mapf_last_error()
    assert (buf[nq:] == 9).all()
    assert set(np.unique(buf[:nq])) <= {0, 1}
    return buf[:nq].astype(bool)


def band_bytes(N, C, F):
    """bool per byte of one env's slice: inside some agent's channel 5."""
    m = np.zeros((N, C, F * F * 4), bool)
    m[:, 5] = True
    return m.reshape(-1)


@pytest.mark.parametrize("N,C,F", SHAPES)
@pytest.mark.parametrize("unit", UNITS)
def test_skip_set_is_whole_aligned_units_inside_the_band(N, C, F, unit):
    band = band_bytes(N, C, F)
    agent_bytes = C * F * F * 4
    for off in OFFSETS:
        skip = skip_bitmap(N, C, F, unit, off)
        sb = np.repeat(skip, 16)                                   # per byte of the slice
        assert not (sb & ~band).any(), (off, "a skipped byte outside the band")
        # runs of skipped bytes: whole units at unit-aligned absolute addresses, inside ONE agent's band
        edges = np.flatnonzero(np.diff(np.concatenate(([0], sb.astype(np.int8), [0]))))
        for a, b in zip(edges[::2], edges[1::2]):
            assert (off + a) % unit == 0 and (b - a) % unit == 0, (off, a, b)
            assert a // agent_bytes == (b - 1) // agent_bytes
        # and nothing skippable is left: every aligned unit wholly inside a band is skipped
        first = (-off) % unit
        for a in range(first, len(band) - unit + 1, unit):
            if band[a:a + unit].all() and a // agent_bytes == (a + unit - 1) // agent_bytes:
                assert sb[a:a + unit].all(), (off, a)
        # only off % unit matters
        np.testing.assert_array_equal(skip, skip_bitmap(N, C, F, unit, off + 5 * 128))
        np.testing.assert_array_equal(skip, skip_bitmap(N, C, F, unit, off % unit))


def test_c2_totals():
    """c2 (8 agents, FOV 11): an env's slice is 23,232 B = 181.5 lines, so env b starts at
    64 * (b & 1) modulo 128.  Band bytes skipped per agent-step, mean over the two parities, of 484."""
    want = {16: 472, 64: 424, 128: 360}
    for unit in UNITS:
        tot = [int(skip_bitmap(8, 6, 11, unit, off).sum()) * 16 for off in (0, 64)]
        assert sum(tot) / 2 / 8 == want[unit], (unit, tot)
    for off in OFFSETS:                                # the 16-B set does not depend on alignment
        np.testing.assert_array_equal(skip_bitmap(8, 6, 11, 16, off), skip_bitmap(8, 6, 11, 16, 0))
        assert int(skip_bitmap(8, 6, 11, 16, off).sum()) == 1452 - 19 * 64      # 19 full instructions remain


@pytest.mark.parametrize("N,C,F", SHAPES)
def test_no_band_no_skips(N, C, F):
    for unit in UNITS + [0]:
        for off in OFFSETS:
            assert not skip_bitmap(N, C, F, unit, off, use_hp=1).any()
    if N * 5 * F * F % 4 == 0:
        assert not skip_bitmap(N, 5, F, 16, 0).any()   # no channel 5 at all


def test_unit_zero_is_the_kernels_unit_whatever_the_batch():
    """unit 0 = the unit the kernel skips in (64 B), also where the slot stride B * env bytes is not
    a multiple of it (B = 37, N = 6, F = 9: 37 * 11664 B), so that the set moves from slot to slot."""
    assert 37 * 6 * 6 * 81 * 4 % 64 != 0
    for (N, C, F), B in zip(SHAPES, (4096, 37, 41)):
        for off in OFFSETS:
            np.testing.assert_array_equal(skip_bitmap(N, C, F, 0, off, B=B), skip_bitmap(N, C, F, 64, off))
    assert any((skip_bitmap(6, 6, 9, 0, off) != skip_bitmap(6, 6, 9, 0, 0)).any() for off in OFFSETS)


def test_bad_arguments_are_rejected():
    from mapf_amd import _lib
    from mapf_amd.config import make_config
    cfg = make_config(4, 20, 20, num_agents=8, fov=11, num_channel=6)
    buf = np.zeros(2000, np.uint8)
    L = _lib.lib()
    assert L.mapf_obs_band_skip(ctypes.byref(cfg), 32, 0, buf.ctypes.data, 2000) == -1
    assert L.mapf_obs_band_skip(ctypes.byref(cfg), 64, 8, buf.ctypes.data, 2000) == -1
    assert L.mapf_obs_band_skip(None, 64, 0, buf.ctypes.data, 2000) == -1
