"""CPU check of the grouped rollout's pacing protocol (csrc/mapf_group.h: pace_gate, pace_word), through
the host side of the one predicate the kernel runs too, exported as mapf_pace_gate.  libmapf.so loads
without a GPU.

16 waves of one workgroup are simulated under random interleavings: a wave that wants to start step t
asks the gate for its ring word and target, starts if the word has reached the target, and adds 1 to
word pace_word(t) when it finishes step t -- exactly the kernel's reads and writes, one at a time (LDS
reads and atomic adds of one workgroup are sequentially consistent).  At every event: no wave is more
than `slack` steps ahead of the slowest live wave, and some wave can always move (no deadlock: a wrong
wait is a GPU hang)."""
import ctypes

import numpy as np
import pytest

RING = 16
WAVES = 16


def gate(t, slack, live):
    from mapf_amd import _lib
    word, target = ctypes.c_int32(-1), ctypes.c_uint32(0)
    r = _lib.lib().mapf_pace_gate(t, slack, live, ctypes.byref(word), ctypes.byref(target))
    assert r in (0, 1), _lib.lib().mapf_last_error()
    return bool(r), word.value, target.value


def simulate(T, slack, live, rng, bias):
    """bias: per-wave weights of being scheduled next (a slow wave is one rarely picked)."""
    ring = [0] * RING
    done = [0] * live             # steps finished by each live wave (waves past B never pace or arrive)
    running = [False] * live      # inside step done[w]
    events = 0
    while min(done) < T:
        # the waves that can make a move now
        movable = []
        for w in range(live):
            if done[w] == T:
                continue
            if running[w]:
                movable.append(w)
                continue
            need, word, target = gate(done[w], slack, live)
            if need:
                assert 0 <= word < RING
            if not need or ring[word] >= target:
                movable.append(w)
            # a wave that would wait: it may be at most `slack` ahead, and must not be the slowest
            else:
                assert done[w] > min(done), (done, w, "the slowest wave waits: deadlock")
        assert movable, (done, ring, "no wave can move")
        p = np.array([bias[w] for w in movable], float)
        w = movable[rng.choice(len(movable), p=p / p.sum())]
        if running[w]:
            ring[done[w] % RING] += 1
            assert done[w] % RING == pace_word(done[w])
            done[w] += 1
            running[w] = False
        else:
            running[w] = True
            # the wave is now inside step done[w]: the slowest has finished done[w] - slack at least
            assert done[w] - min(done) <= min(slack, RING - 2), (done, w, slack)
        assert max(d + r for d, r in zip(done, running)) - 1 - min(done) <= min(slack, RING - 2)
        events += 1
    assert events == 2 * T * live
    # the words end at live * laps: nothing was lost or counted twice
    for k in range(RING):
        assert ring[k] == live * len(range(k, T, RING))


def pace_word(t):
    need, word, _ = gate(t + 1, 0, 1)      # the gate of step t + 1 at slack 0 reads step t's word
    assert need
    return word


@pytest.mark.parametrize("live", [16, 13])
@pytest.mark.parametrize("slack", [0, 1, 3])
def test_random_interleavings_never_run_ahead_and_never_deadlock(slack, live):
    rng = np.random.default_rng(100 * slack + live)
    for T in (1, 2, 17, 40):
        simulate(T, slack, live, rng, [1.0] * live)                       # fair scheduling
        simulate(T, slack, live, rng, [0.02] + [1.0] * (live - 1))        # one trailing wave
        simulate(T, slack, live, rng, list(rng.uniform(0.05, 1.0, live)))


def test_gate_arithmetic():
    for slack in (0, 1, 3):
        for live in (16, 13, 1):
            for t in range(0, 40):
                need, word, target = gate(t, slack, live)
                u = t - slack - 1
                assert need == (u >= 0)
                if need:
                    assert word == u % RING and target == live * (u // RING + 1)
    # a slack the ring cannot hold is paced at the ring's limit
    assert gate(20, 1 << 20, 16) == gate(20, RING - 2, 16)


def test_more_slack_than_the_ring_holds_is_still_safe():
    rng = np.random.default_rng(7)
    simulate(40, 1 << 20, 16, rng, [0.02] + [1.0] * 15)


def test_bad_arguments_are_rejected():
    from mapf_amd import _lib
    L = _lib.lib()
    w, t = ctypes.c_int32(0), ctypes.c_uint32(0)
    assert L.mapf_pace_gate(-1, 1, 16, ctypes.byref(w), ctypes.byref(t)) < 0
    assert L.mapf_pace_gate(1, -1, 16, ctypes.byref(w), ctypes.byref(t)) < 0      # pacing off: no gate to ask
    assert L.mapf_pace_gate(1, 1, 0, ctypes.byref(w), ctypes.byref(t)) < 0
    assert L.mapf_pace_gate(1, 1, 65, ctypes.byref(w), ctypes.byref(t)) < 0
    assert L.mapf_pace_gate(1, 1, 16, None, ctypes.byref(t)) < 0
