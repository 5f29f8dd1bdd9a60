"""BatchedMapfGym: B lockstep MAPF environments resident on one MI355X.

Python face of libmapf.so (include/mapf.h).  Every call is asynchronous on
the current torch HIP stream; inputs and outputs are torch tensors in HBM.
Reference API it batches: mapf_gym.MapfGym / FixedMapfGym (mapf_gym.py:163-669).
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from .config import MapfConfig, make_config


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check(t, dtype, numel, device, name):
    """Every buffer handed to the kernels as a raw pointer: right dtype, contiguous,
    the element count the kernel writes, on the handle's GPU (a wrong one would be
    an out-of-bounds device write, not an error)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if t.numel() != numel:
        raise ValueError(f"{name}: {t.numel()} elements, expected {numel}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    return t


def parse_tuning(text):
    """ "roll_fair=2,wide_obs=1" -> {"roll_fair": 2, "wide_obs": 1} (mapf_tuning fields)."""
    out = {}
    for kv in (text or "").split(","):
        if kv.strip():
            k, v = kv.split("=")
            out[k.strip()] = int(v)
    return out


# rollout policy (its name in the plan texts: ",tape", ",descent", ",pibt") -> the library's (rollout, plan) calls
ROLLOUT_POLICIES = {"random": ("mapf_rollout_random", "mapf_rollout_plan"),
                    "tape": ("mapf_rollout_actions", "mapf_rollout_actions_plan"),
                    "descent": ("mapf_rollout_descent", "mapf_rollout_descent_plan"),
                    "pibt": ("mapf_rollout_pibt", "mapf_rollout_pibt_plan")}


def _policy_symbols(policy):
    if policy not in ROLLOUT_POLICIES:
        raise ValueError(f"policy: expected one of {sorted(ROLLOUT_POLICIES)}, got {policy!r}")
    return ROLLOUT_POLICIES[policy]


def noise_q16(eps=None, q16=None):
    """Action noise as the library takes it (mapf_set_action_noise): eps, a float in [0, 1], gives
    round(eps * 65536); or q16=, the integer in 0..65536, directly."""
    if (eps is None) == (q16 is None):
        raise ValueError("action noise: give eps or q16=, one of them")
    if q16 is not None:
        if isinstance(q16, bool) or not isinstance(q16, (int, np.integer)):
            raise TypeError(f"action noise q16: expected an int in 0..65536, got {type(q16).__name__}")
        if not 0 <= int(q16) <= 65536:
            raise ValueError(f"action noise q16 must be in 0..65536, got {int(q16)}")
        return int(q16)
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise TypeError(f"action noise eps: expected a float in [0, 1], got {type(eps).__name__}")
    if not 0.0 <= float(eps) <= 1.0:        # (NaN fails both)
        raise ValueError(f"action noise eps must be in [0, 1], got {eps!r}")
    return int(round(float(eps) * 65536))


def _check_noise_policy(policy, noise):
    """noise= of a rollout call: None, or an eps for the picked policies; returns its q16 (None: leave alone)."""
    if noise is None:
        return None
    if policy not in ("descent", "pibt"):
        raise ValueError(f"noise= goes with policy 'descent' or 'pibt', not {policy!r}")
    return noise_q16(noise)


# mapf_rollout_sparse's policy argument (include/mapf.h)
SPARSE_POLICY = {"random": 0, "tape": 1, "descent": 2, "pibt": 3}


def sparse_applies(N, C, F, address):
    """mapf_obs_sparse_applies (include/mapf.h) without the call: an env's observation slice is a whole
    number of 64-byte pieces that 16 mask words can name, and the buffer is 64-byte aligned."""
    floats = N * C * F * F
    return floats > 0 and floats % 16 == 0 and floats // 16 <= 512 and address % 64 == 0


class _SparseEntry:
    """What the sparse launchers over one observation buffer share (rollout_launcher): the shadow
    masks int32 [slots][B][16] of mapf_rollout_sparse, the number of leading slots they describe,
    and obs._version as it was after the last launch (torch counts its own in-place writes there,
    for every view of the buffer; a launch through the raw pointer does not count)."""
    __slots__ = ("shadow", "valid", "version", "geometry", "__weakref__")

    def __init__(self, shadow, version, geometry):
        self.shadow, self.valid, self.version, self.geometry = shadow, 0, version, geometry


# (device, base address of the obs tensor's storage) -> _SparseEntry, alive as long as a launcher holds it
# (each launcher also holds its buffers, so the address is not handed out again under a live entry)
_SPARSE = weakref.WeakValueDictionary()


def _sparse_key(obs):
    return (str(obs.device), obs.untyped_storage().data_ptr())


def _sparse_forget(obs):
    """Another rollout call writes `obs`: a registered buffer's shadow no longer describes it."""
    if _SPARSE and isinstance(obs, torch.Tensor):
        entry = _SPARSE.get(_sparse_key(obs))
        if entry is not None:
            entry.valid = 0


class BatchedMapfGym:
    """B environments x N agents on one GPU (one handle per process/GPU)."""

    def __init__(self, cfg: MapfConfig = None, device=None, tuning=None, **kw):
        """tuning: optional mapf_tuning fields (include/mapf.h) as a dict or a "k=v,k=v" string --
        which form of a kernel the launches take; results are identical for every value
        (see set_tuning)."""
        if isinstance(tuning, str):
            tuning = parse_tuning(tuning)
        if cfg is None:
            cfg = make_config(**kw)
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedMapfGym needs a GPU (MI355X); there is no CPU fallback")
        self.cfg = cfg
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.B, self.N, self.H, self.W = cfg.num_envs, cfg.num_agents, cfg.height, cfg.width
        self.F, self.C = cfg.fov, cfg.num_channel
        self.obs_words = int(_lib.lib().mapf_obs_bits_words(ctypes.byref(cfg)))   # WPA: uint32 words per packed agent
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mapf_create(ctypes.byref(cfg), self.device.index, ctypes.byref(h)))
        self.h = h
        self.path_capacity = _lib.lib().mapf_path_capacity(self.h)
        if tuning:
            self.set_tuning(**tuning)
        else:
            self._query_forms()
        dev = self.device
        B, N = self.B, self.N
        self.out = dict(
            status=torch.zeros(B, N, dtype=torch.int8, device=dev),
            reward=torch.zeros(B, N, dtype=torch.float32, device=dev),
            shadow_goals=torch.zeros(B, dtype=torch.int32, device=dev),
            cost=torch.zeros(B, N, dtype=torch.float32, device=dev),
            train_valid=torch.zeros(B, N, 5, dtype=torch.float32, device=dev),
            actions_fixed=torch.zeros(B, N, dtype=torch.int32, device=dev),
            goals_reached=torch.zeros(B, N, dtype=torch.float32, device=dev),
            constraints=torch.zeros(B, N, dtype=torch.float32, device=dev),
            reward_total=torch.zeros(B, N, dtype=torch.float32, device=dev))
        self._stepout = self._make_stepout(self.out)
        self.obs = torch.zeros(B, N, self.C, self.F, self.F, dtype=torch.float32, device=dev)
        self.vec = torch.zeros(B, N, 4, dtype=torch.float32, device=dev)
        self.actions = torch.zeros(B, N, dtype=torch.int32, device=dev)

    def _query_forms(self):
        self.fused = bool(_lib.lib().mapf_step_observe_fused(self.h))   # step_observe = one launch
        # rollout_random = one launch: 1 pair-lane kernel (c2), 2 one wave per env (c4, c5); 0 per-step launches
        self.rollout_kernel = int(_lib.lib().mapf_rollout_random_fused(self.h))
        self.rollout_fused = self.rollout_kernel != 0
        self._roll_fast = None

    @staticmethod
    def default_tuning():
        """mapf_tuning_default as a dict (include/mapf.h: mapf_tuning)."""
        t = _lib.Tuning()
        _lib.lib().mapf_tuning_default(ctypes.byref(t))
        return {n: int(getattr(t, n)) for n in _lib.TUNING_FIELDS}

    def tuning(self):
        t = _lib.Tuning()
        _lib.check(_lib.lib().mapf_get_tuning(self.h, ctypes.byref(t)))
        return {n: int(getattr(t, n)) for n in _lib.TUNING_FIELDS}

    def set_tuning(self, **fields):
        """Change launch-form fields of mapf_tuning (unknown names raise, bad values raise
        through the library's validation); the next launch takes the new form."""
        t = _lib.Tuning()
        _lib.check(_lib.lib().mapf_get_tuning(self.h, ctypes.byref(t)))
        for k, v in fields.items():
            if k not in _lib.TUNING_FIELDS:
                raise KeyError(f"unknown tuning field {k!r}")
            setattr(t, k, int(v))
        _lib.check(_lib.lib().mapf_set_tuning(self.h, ctypes.byref(t)))
        self._query_forms()

    @staticmethod
    def _slot_bits(slots, band_clean, obs_bits=False):
        """The `slots` argument of the mapf_rollout_* calls (MAPF_SLOTS_*, mapf.h)."""
        return ((_lib.SLOTS | (_lib.SLOTS_BAND_CLEAN if band_clean else 0)) if slots else 0) | \
            (_lib.SLOTS_OBS_BITS if obs_bits else 0)

    def rollout_plan(self, slots=False, band_clean=False, obs_bits=False, *, policy="random"):
        """The kernel (template instantiation + form) a rollout under `policy` launches now, as text
        (the policy's mapf_rollout_*plan call).  band_clean: for a slots launch with MAPF_SLOTS_BAND_CLEAN;
        obs_bits: for a packed launch, MAPF_SLOTS_OBS_BITS -- ",bits" inside the angle brackets.  A policy
        other than "random" comes last inside them (",tape", ",descent", ",pibt"; descent and pibt take the
        wide three-wave form with bfsobs=0); where the call runs per-step launches the text is "step_observe",
        "descent_actions+step_observe" or "pibt_actions+step_observe".  mapf.h lists the kernels' symbols."""
        fn = getattr(_lib.lib(), _policy_symbols(policy)[1])
        buf = ctypes.create_string_buffer(512)
        kind = fn(self.h, self._slot_bits(slots, band_clean, obs_bits), buf, 512)
        if kind < 0:
            _lib.check(kind)
        return buf.value.decode()

    def rollout_kernel_name(self, slots=False, obs_bits=False, *, band_clean=False, policy="random"):
        """The template instantiation alone, e.g. 'rollout_wide3_kernel<u64,1,true,tape>' under "tape"."""
        return self.rollout_plan(slots, band_clean, obs_bits, policy=policy).split(" ")[0]

    def rollout_actions_plan(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_plan(policy="tape")."""
        return self.rollout_plan(slots, band_clean, obs_bits, policy="tape")

    def rollout_actions_kernel_name(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_kernel_name(policy="tape")."""
        return self.rollout_kernel_name(slots, obs_bits, band_clean=band_clean, policy="tape")

    def rollout_descent_plan(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_plan(policy="descent")."""
        return self.rollout_plan(slots, band_clean, obs_bits, policy="descent")

    def rollout_descent_kernel_name(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_kernel_name(policy="descent")."""
        return self.rollout_kernel_name(slots, obs_bits, band_clean=band_clean, policy="descent")

    def rollout_pibt_plan(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_plan(policy="pibt")."""
        return self.rollout_plan(slots, band_clean, obs_bits, policy="pibt")

    def rollout_pibt_kernel_name(self, slots=False, band_clean=False, obs_bits=False):
        """rollout_kernel_name(policy="pibt")."""
        return self.rollout_kernel_name(slots, obs_bits, band_clean=band_clean, policy="pibt")

    @staticmethod
    def _make_stepout(out):
        so = _lib.StepOut()
        for name, _ in _lib.StepOut._fields_:
            t = out.get(name)
            setattr(so, name, t.data_ptr() if t is not None else None)
        return so

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().mapf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- reset
    def _maps_array(self, maps):
        maps = np.ascontiguousarray(maps, dtype=np.int8)
        if self.cfg.shared_map:
            maps = maps.reshape(1, self.H, self.W)
        else:
            maps = maps.reshape(self.B, self.H, self.W)
        return maps

    def reset_fixed(self, maps, seqs, human_start=None, human_goal=None, human_seq=None):
        """FixedMapfGym (mapf_gym.py:648-669) for every env.

        seqs: [B][N] lists of (row, col) -- start then goals (util.Sequence).
        human_start/goal: [B, 2] (LoopingHuman) or human_seq: [B] lists (FixedPathHuman)."""
        m = self._maps_array(maps)
        S = self.cfg.max_seq
        seq = np.zeros((self.B, self.N, S, 2), np.int32)
        sl = np.zeros((self.B, self.N), np.int32)
        for b in range(self.B):
            for i in range(self.N):
                s = np.asarray(seqs[b][i], np.int32).reshape(-1, 2)
                if len(s) > S:
                    raise ValueError(f"sequence of {len(s)} cells exceeds max_seq={S}")
                seq[b, i, :len(s)] = s
                sl[b, i] = len(s)
        spec = _lib.ResetSpec()
        spec.mode = 0
        keep = [m, seq, sl]
        spec.maps = m.ctypes.data
        spec.seq = seq.ctypes.data
        spec.seq_len = sl.ctypes.data
        if human_seq is not None:
            HS = self.cfg.max_human_seq
            hs = np.zeros((self.B, HS, 2), np.int32)
            hl = np.zeros(self.B, np.int32)
            for b in range(self.B):
                q = np.asarray(human_seq[b], np.int32).reshape(-1, 2)
                hs[b, :len(q)] = q
                hl[b] = len(q)
            keep += [hs, hl]
            spec.human_seq = hs.ctypes.data
            spec.human_seq_len = hl.ctypes.data
        else:
            a = np.ascontiguousarray(np.asarray(human_start, np.int32).reshape(self.B, 2))
            g = np.ascontiguousarray(np.asarray(human_goal, np.int32).reshape(self.B, 2))
            keep += [a, g]
            spec.human_start = a.ctypes.data
            spec.human_goal = g.ctypes.data
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mapf_reset(self.h, ctypes.byref(spec), _stream(self.device)))
        del keep

    def reset_seeded(self, maps, seed=0):
        """MapfGym (mapf_gym.py:164-184): human entrance/goal and agent starts/goals drawn on device."""
        m = self._maps_array(maps)
        spec = _lib.ResetSpec()
        spec.mode = 1
        spec.maps = m.ctypes.data
        spec.seed = seed
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mapf_reset(self.h, ctypes.byref(spec), _stream(self.device)))

    def reset_generated(self, kind="warehouse", lo=None, hi=None, density=0.3, largest=False, epoch=0, seed=0,
                        return_maps=False):
        """MapfGym() on maps generated on the device (mapf_reset_generated): kind "warehouse"
        draws each env's generateWarehouse length in [lo, hi] (default EnvParameters.WORLD_SIZE,
        mapf_gym.py:166; the H x W stack must hold the longest), "random" fills H x W with
        -(rand < density); largest keeps the largest 4-connected free component.  Then the
        seeded reset (agents, goals, human) as reset_seeded.  Asynchronous; return_maps gives
        the int8 maps as a device tensor [shared_map ? 1 : B, H, W]."""
        from .config import EnvParameters
        spec = _lib.MapGenSpec()
        spec.kind = {"warehouse": _lib.MAPS_WAREHOUSE, "random": _lib.MAPS_RANDOM}[kind]
        ws = EnvParameters.WORLD_SIZE
        spec.lo = ws[0] if lo is None else lo
        spec.hi = ws[1] if hi is None else hi
        spec.largest, spec.density, spec.epoch, spec.seed = int(largest), float(density), int(epoch), int(seed)
        maps = None
        if return_maps:
            maps = torch.empty(1 if self.cfg.shared_map else self.B, self.H, self.W, dtype=torch.int8,
                               device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mapf_reset_generated(self.h, ctypes.byref(spec), _ptr(maps),
                                                       _stream(self.device)))
        return maps

    # ----------------------------------------------------------------- step
    def step(self, actions=None, commit=True):
        """One lockstep step (runner.py:64-100 order).  actions: int32 [B, N] on device.
        Returns the dict of output tensors (reused between calls).

        Graph capture: steps and observes may be captured into a hipGraph and
        replayed, provided a captured sequence holds a multiple of 3 committed
        steps (the device work lists rotate over 3 slots)."""
        if actions is None:
            actions = self.actions
        _check(actions, torch.int32, self.B * self.N, self.device, "actions")
        _lib.check(_lib.lib().mapf_step(self.h, _ptr(actions), ctypes.byref(self._stepout),
                                        1 if commit else 0, _stream(self.device)))
        return self.out

    def step_random(self, actions=None, commit=True):
        """Random-policy step: actions drawn on device (written to `actions`), then stepped, one launch."""
        if actions is None:
            actions = self.actions
        _check(actions, torch.int32, self.B * self.N, self.device, "actions")
        _lib.check(_lib.lib().mapf_step_random(self.h, _ptr(actions), ctypes.byref(self._stepout),
                                               1 if commit else 0, _stream(self.device)))
        return self.out

    def observe(self, obs=None, vec=None):
        """getAllObservations for all envs: obs [B, N, C, F, F], vec [B, N, 4] (float32)."""
        obs = self.obs if obs is None else obs
        vec = self.vec if vec is None else vec
        _check(obs, torch.float32, self.B * self.N * self.C * self.F * self.F, self.device, "obs")
        _check(vec, torch.float32, self.B * self.N * 4, self.device, "vec")
        _lib.check(_lib.lib().mapf_observe(self.h, _ptr(obs), _ptr(vec), _stream(self.device)))
        return obs, vec

    def _bits_buffer(self, bits, k=1):
        """A packed observation buffer: int32 [k*B, N, WPA] elements (the default: this env's own
        [B, N, WPA], allocated on first use)."""
        if bits is None:
            if getattr(self, "bits", None) is None:
                self.bits = torch.zeros(self.B, self.N, self.obs_words, dtype=torch.int32, device=self.device)
            bits = self.bits
        return _check(bits, torch.int32, k * self.B * self.N * self.obs_words, self.device, "bits")

    def observe_bits(self, bits=None, vec=None):
        """observe() writing the packed observation (mapf_observe_bits): bits int32 [B, N, WPA]
        (WPA = obs_words; one bit per cell, unpack_obs gives the floats back), vec [B, N, 4]."""
        bits = self._bits_buffer(bits)
        vec = self.vec if vec is None else vec
        _check(vec, torch.float32, self.B * self.N * 4, self.device, "vec")
        _lib.check(_lib.lib().mapf_observe_bits(self.h, _ptr(bits), _ptr(vec), _stream(self.device)))
        return bits, vec

    def step_observe_bits(self, actions=None, bits=None, vec=None, out=None):
        """step_observe() writing the packed observation (mapf_step_observe_bits).
        Returns (out, bits, vec)."""
        if actions is None:
            actions = self.actions
        bits = self._bits_buffer(bits)
        vec = self.vec if vec is None else vec
        _check(actions, torch.int32, self.B * self.N, self.device, "actions")
        _check(vec, torch.float32, self.B * self.N * 4, self.device, "vec")
        so = self._stepout if out is None else self._make_stepout(self._check_out(out))
        _lib.check(_lib.lib().mapf_step_observe_bits(self.h, _ptr(actions), ctypes.byref(so), _ptr(bits), _ptr(vec),
                                                     _stream(self.device)))
        return (self.out if out is None else out), bits, vec

    def step_observe(self, actions=None, obs=None, vec=None, random_policy=False, out=None):
        """Committed step + getAllObservations in one launch (mapf_step_observe): the same
        outputs as step() followed by observe().  random_policy: draw the actions on device
        into `actions` first (mapf_step_observe_random).  out: optional dict of output
        tensors (the keys of self.out, any subset; missing = not written) to write the step's
        outputs into instead of self.out, e.g. slices of rollout buffers.
        Returns (out, obs, vec)."""
        if actions is None:
            actions = self.actions
        obs = self.obs if obs is None else obs
        vec = self.vec if vec is None else vec
        _check(actions, torch.int32, self.B * self.N, self.device, "actions")
        _check(obs, torch.float32, self.B * self.N * self.C * self.F * self.F, self.device, "obs")
        _check(vec, torch.float32, self.B * self.N * 4, self.device, "vec")
        fn =_lib.lib().mapf_step_observe_random if random_policy else _lib.lib().mapf_step_observe
        so = self._stepout if out is None else self._make_stepout(self._check_out(out))
        _lib.check(fn(self.h, _ptr(actions), ctypes.byref(so), _ptr(obs), _ptr(vec), _stream(self.device)))
        return (self.out if out is None else out), obs, vec

    def rollout(self, T=None, policy="random", *, slots=False, actions=None, tape=None, obs=None, vec=None, out=None,
                band_clean=False, obs_bits=False, noise=None):
        """T x (the policy's actions, step_observe) -- runner.py:64-100, T times -- as ONE launch where
        rollout_fused (each wave owns an env and loops step -> observe -> its search work; the kernel
        is rollout_plan(policy=...)), else per-step launches; identical results.  policy:
          "random"   uniform random, drawn in the kernel (mapf_rollout_random);
          "tape"     the caller's policy (mapf_rollout_actions): tape int32 [T, B, N] on the device,
                     read by the launch (not by this call), always [T]-leading, T = tape.shape[0];
                     values outside 0..4 are counted as bad actions and played as 0;
                     out["actions_fixed"] is what was executed and must not overlap the tape;
          "descent"  the heuristic baseline, every agent one step down its own BFS map (needs keep_bfs);
          "pibt"     the collision-free baseline, the PIBT planner (needs keep_bfs), its ages included.
        `actions` receives the drawn or chosen actions (not used under "tape").  slots: step t writes
        slot t of [T]-leading buffers (actions [T, B, N], obs [T, B, N, C, F, F], vec [T, B, N, 4],
        out[k] [T, ...]); otherwise every step overwrites the [B]-leading buffers.
        band_clean (with slots): the caller's promise that the zero band of every slot of `obs`
        (channel 5 while use_hp is off) already holds zeros, e.g. from an earlier call on the same
        buffer without it; the launch then need not store it (MAPF_SLOTS_BAND_CLEAN, mapf.h).
        obs_bits: `obs` is the packed observation buffer, int32 [T, B, N, WPA] (slots) or [B, N, WPA]
        (default: this env's own), one bit per cell (MAPF_SLOTS_OBS_BITS; band_clean is then ignored).
        noise ("descent" / "pibt" only, ValueError otherwise): an eps in [0, 1] set on the handle before
        the launch (set_action_noise); None leaves the handle's setting alone.  `actions` keeps the
        policy's picks, the labels; the steps play the noisy actions.
        Returns (out, obs, vec)."""
        symbol = _policy_symbols(policy)[0]
        q16 = _check_noise_policy(policy, noise)
        if policy == "tape":
            n = self._check_tape(tape)
            if T is not None and int(T) != n:
                raise ValueError(f"T = {T} but the tape holds {n} steps")
            T = n
        elif tape is not None:
            raise ValueError(f"tape= goes with policy='tape', not {policy!r}")
        elif policy != "random":
            T = int(T)
            if T < 0:
                raise ValueError("T must be >= 0")
        actions, so, out, obs, vec = self._rollout_buffers(T if slots else 1, slots, obs, vec, out, actions=actions,
                                                           tape=tape, obs_bits=obs_bits)
        if q16 is not None:
            self.set_action_noise(q16=q16)
        if T == 0 and policy != "random":   # nothing to play (an empty tensor has no address to hand over)
            return out, obs, vec
        _sparse_forget(obs)
        _lib.check(getattr(_lib.lib(), symbol)(self.h, int(T), self._slot_bits(slots, band_clean, obs_bits), _ptr(actions),
                                               ctypes.byref(so), _ptr(obs), _ptr(vec), _stream(self.device)))
        return out, obs, vec

    def rollout_random(self, T, slots=False, actions=None, obs=None, vec=None, out=None, band_clean=False,
                       obs_bits=False):
        """rollout(T, "random", ...); the default in-place call takes the cached-argument path below."""
        if not obs_bits and not slots and actions is None and obs is None and vec is None and out is None:
            # the default [B]-leading buffers (checked at construction): the call's arguments are
            # built once -- a 20-step rollout takes ~300 us on the GPU, so the host's ~8 us of
            # argument checks and ctypes wrapping per call were 2-3 % of it
            key = (id(self.h), id(self.actions), id(self.obs), id(self.vec), id(self._stepout))
            fast = self._roll_fast
            if fast is None or fast[0] != key:
                fast = self._roll_fast = (key, _lib.lib().mapf_rollout_random, self.h, ctypes.byref(self._stepout),
                                          _ptr(self.actions), _ptr(self.obs), _ptr(self.vec))
            _, fn, h, so, pa, po, pv = fast
            _sparse_forget(self.obs)
            _lib.check(fn(h, int(T), 0, pa, so, po, pv, _stream(self.device)))
            return self.out, self.obs, self.vec
        return self.rollout(T, "random", slots=slots, actions=actions, obs=obs, vec=vec, out=out, band_clean=band_clean,
                            obs_bits=obs_bits)

    def _check_tape(self, tape, T=None):
        """An action tape: int32 [T, B, N], contiguous, on the handle's GPU (the kernels read it
        through a raw pointer).  Returns T."""
        if not isinstance(tape, torch.Tensor):
            raise TypeError(f"tape: expected a torch.Tensor, got {type(tape).__name__}")
        if tape.dim() != 3 or tuple(tape.shape[1:]) != (self.B, self.N) or (T is not None and tape.shape[0] != T):
            raise ValueError(f"tape: shape {tuple(tape.shape)}, expected [{'T' if T is None else T}, {self.B}, {self.N}]")
        _check(tape, torch.int32, tape.shape[0] * self.B * self.N, self.device, "tape")
        return int(tape.shape[0])

    def _rollout_buffers(self, k, slots, obs, vec, out, actions=None, tape=None, obs_bits=False):
        """The buffers of a rollout call (k = T with slots, else 1), defaulted and checked in the order
        actions, obs, vec, out: (actions, so, out, obs, vec).  tape: a tape _check_tape has passed,
        handed back in the actions' place.  obs_bits: obs is the packed int32 [k*B, N, WPA] buffer."""
        if tape is not None:
            actions = tape
        else:
            actions = self.actions if actions is None else actions
            _check(actions, torch.int32, k * self.B * self.N, self.device, "actions")
        vec = self.vec if vec is None else vec
        if obs_bits:
            obs = self._bits_buffer(obs, k)
        else:
            obs = self.obs if obs is None else obs
            _check(obs, torch.float32, k * self.B * self.N * self.C * self.F * self.F, self.device, "obs")
        _check(vec, torch.float32, k * self.B * self.N * 4, self.device, "vec")
        if out is None:
            if slots:
                raise ValueError("slots=True needs [T]-leading output buffers (out=...)")
            return actions, self._stepout, self.out, obs, vec
        for key, t in out.items():
            ref = self.out[key]
            _check(t, ref.dtype, k * ref.numel(), self.device, key)
        return actions, self._make_stepout(out), out, obs, vec

    def rollout_actions(self, tape, slots=False, obs=None, vec=None, out=None, band_clean=False, obs_bits=False):
        """rollout(policy="tape", tape=tape, ...)."""
        return self.rollout(None, "tape", slots=slots, tape=tape, obs=obs, vec=vec, out=out, band_clean=band_clean,
                            obs_bits=obs_bits)

    def rollout_descent(self, T, slots=False, actions=None, obs=None, vec=None, out=None, band_clean=False,
                        obs_bits=False):
        """rollout(T, "descent", ...)."""
        return self.rollout(T, "descent", slots=slots, actions=actions, obs=obs, vec=vec, out=out, band_clean=band_clean,
                            obs_bits=obs_bits)

    def rollout_pibt(self, T, slots=False, actions=None, obs=None, vec=None, out=None, band_clean=False,
                     obs_bits=False):
        """rollout(T, "pibt", ...)."""
        return self.rollout(T, "pibt", slots=slots, actions=actions, obs=obs, vec=vec, out=out, band_clean=band_clean,
                            obs_bits=obs_bits)

    def rollout_sparse(self, T, policy="random", *, shadow, valid, actions=None, tape=None, obs, vec, out):
        """mapf_rollout_sparse (mapf.h): rollout(T, policy, slots=True, ...) that stores only the 64-byte
        observation pieces that change.  shadow: int32 [T, B, 16] on the device, the caller's piece masks
        of `obs`; valid: the leading slots for which the caller vouches that they describe what `obs`
        holds now (0: none).  The launch leaves the slots' new masks in `shadow`.  rollout_launcher does
        this bookkeeping by itself.  Returns (out, obs, vec)."""
        _policy_symbols(policy)
        T = self._check_tape(tape) if policy == "tape" else int(T)
        actions, so, out, obs, vec = self._rollout_buffers(T, True, obs, vec, out, actions=actions,
                                                           tape=tape if policy == "tape" else None)
        _check(shadow, torch.int32, T * self.B * 16, self.device, "shadow")
        if T == 0:
            return out, obs, vec
        _sparse_forget(obs)
        _lib.check(_lib.lib().mapf_rollout_sparse(self.h, SPARSE_POLICY[policy], T, _ptr(actions), ctypes.byref(so),
                                                  _ptr(obs), _ptr(vec), _ptr(shadow), int(valid), _stream(self.device)))
        return out, obs, vec

    def rollout_perf(self, T=None, policy="random", *, tape=None, actions=None, perf=None, accumulate=False, noise=None):
        """mapf_rollout_perf (mapf.h): T committed steps under `policy` (rollout's names; T / tape as there) in
        one launch that writes only the episode metrics -- no observation, no vec, no step output.  Returns
        perf, int32 [B, 8] on the device (perf_dict names the columns; the two float columns hold float32
        bits), newly allocated if None.  accumulate: continue from what `perf` holds (the float sums go on
        in order: any chunking of an episode gives the bits of one launch).  actions: None, or int32
        [T, B, N] receiving the drawn / chosen actions (not used under "tape").  noise: as rollout()'s.  The
        handle ends exactly as after rollout(T, policy, ...)."""
        _policy_symbols(policy)
        q16 = _check_noise_policy(policy, noise)
        if policy == "tape":
            n = self._check_tape(tape)
            if T is not None and int(T) != n:
                raise ValueError(f"T = {T} but the tape holds {n} steps")
            T, actions = n, tape
        elif tape is not None:
            raise ValueError(f"tape= goes with policy='tape', not {policy!r}")
        else:
            T = int(T)
            if T < 0:
                raise ValueError("T must be >= 0")
            if actions is not None:
                _check(actions, torch.int32, T * self.B * self.N, self.device, "actions")
        if perf is None:
            if accumulate:
                raise ValueError("accumulate=True needs the perf to continue from")
            perf = torch.zeros(self.B, 8, dtype=torch.int32, device=self.device)
        else:
            _check(perf, torch.int32, self.B * 8, self.device, "perf")
        if q16 is not None:
            self.set_action_noise(q16=q16)
        if T == 0:
            return perf
        _lib.check(_lib.lib().mapf_rollout_perf(self.h, SPARSE_POLICY[policy], T, _ptr(actions), _ptr(perf),
                                                1 if accumulate else 0, _stream(self.device)))
        return perf

    def rollout_perf_plan(self, policy="random"):
        """The form a rollout_perf launch takes, as text (mapf_rollout_perf_plan): the kernels' names with
        ",perf" inside the angle brackets, or "<pick>+step+perf_accumulate" for the per-step route."""
        _policy_symbols(policy)
        buf = ctypes.create_string_buffer(512)
        kind = _lib.lib().mapf_rollout_perf_plan(self.h, SPARSE_POLICY[policy], buf, 512)
        if kind < 0:
            _lib.check(kind)
        return buf.value.decode()

    def rollout_sparse_plan(self, obs, policy="random"):
        """The form a mapf_rollout_sparse launch into `obs` takes, as text (mapf_rollout_sparse_plan):
        "rollout_random_kernel<true,4,sparse64> ..." where the sparse form applies, else the band form's."""
        _policy_symbols(policy)
        buf = ctypes.create_string_buffer(512)
        kind = _lib.lib().mapf_rollout_sparse_plan(self.h, SPARSE_POLICY[policy], _ptr(obs), buf, 512)
        if kind < 0:
            _lib.check(kind)
        return buf.value.decode()

    def _sparse_entry(self, T, obs):
        """The shared entry of a sparse launcher over `obs` (created on first use), or None where the
        sparse form does not apply or the registry cannot express the view: it must start at its
        storage's first byte, so that its slot t is the buffer's slot t, with this env's geometry."""
        if getattr(self, "rollout_kernel", 0) != 1 or not sparse_applies(self.N, self.C, self.F, obs.data_ptr()):
            return None
        storage = obs.untyped_storage()
        if obs.data_ptr() != storage.data_ptr():
            return None
        geometry = (self.B, self.N, self.C, self.F)
        entry = _SPARSE.get(_sparse_key(obs))
        if entry is not None:
            return entry if entry.geometry == geometry else None
        slot_bytes = self.B * self.N * self.C * self.F * self.F * 4
        slots = max(int(T), storage.nbytes() // slot_bytes)
        entry = _SparseEntry(torch.zeros(slots, self.B, 16, dtype=torch.int32, device=obs.device), obs._version, geometry)
        _SPARSE[_sparse_key(obs)] = entry
        return entry

    def rollout_launcher(self, T, slots=False, actions=None, obs=None, vec=None, out=None, actions_in=None,
                         policy="random", obs_bits=False, sparse=True, noise=None):
        """rollout(T, policy, slots=slots, ...) prepared once: the buffers are checked and the C call's
        arguments built now, on the current stream; the returned callable issues the launch with
        no per-call host work beyond one ctypes call (a 20-step rollout is ~350 us on the GPU, the
        checks and wrapping ~60 us of host time).  The launcher keeps its buffers alive.

        With slots, the launcher's first call stores every float (right for torch.empty buffers
        too); its later calls tell the library that the observation buffer's zero band (channel 5
        while use_hp is off) is already clean, and the kernel leaves those stores out
        (MAPF_SLOTS_BAND_CLEAN, mapf.h).  The contract: between calls of one launcher nobody writes
        non-zeros into that band of `obs`.  Whoever does (or hands the memory to something that
        may) calls launch.invalidate(): the next call stores everything again.

        sparse (the default, with slots and float observations): where the pair-lane kernel runs and an
        env's observation slice is whole 64-byte pieces (N = 8 with an even channel count: c2), the
        launcher goes further (mapf_rollout_sparse, mapf.h).  It keeps one bit per piece of every slot
        on the device, shared by all launchers over the same buffer (views included, e.g. obs[:n]), and
        a call stores only the pieces that held a non-zero after the previous call or hold one now;
        the buffer ends byte for byte as if everything had been stored.  The launcher notices writes
        made through torch (obs._version, shared by all views): the call after one uses the band form
        above and the next stores everything again.  Any other rollout call of this module into the
        buffer does the same.  The widened contract: whoever writes `obs` behind torch's back between
        calls (raw pointers, another library) calls launch.invalidate().  sparse=False keeps the band
        form alone.  A view that does not start at its storage's first byte gets the band form.

        actions_in: an int32 [T, B, N] tape -- the launcher then issues the "tape" policy over it (`actions`
        is not used); its contents are read at launch time: refill the tensor to play other actions.
        policy: "random" (the default), "descent" or "pibt", as rollout(); these and actions_in exclude
        each other.  The band rule holds for every policy.

        obs_bits: `obs` is the packed int32 buffer (as rollout()); every call stores every word
        (the band rule does not apply).

        noise ("descent" / "pibt" only): an eps set on the handle now, once (set_action_noise); the
        launches read the handle's setting when they are issued, a captured one keeps its capture's."""
        _policy_symbols(policy)
        q16 = _check_noise_policy("tape" if actions_in is not None else policy, noise)
        if actions_in is not None:
            if policy not in ("random", "tape"):
                raise ValueError("policy and actions_in are mutually exclusive")
            policy = "tape"
            self._check_tape(actions_in, int(T))
        elif policy == "tape":
            raise ValueError("policy='tape' needs its tape: actions_in=...")
        actions, so, out, obs, vec = self._rollout_buffers(T if slots else 1, slots, obs, vec, out, actions=actions,
                                                           tape=actions_in, obs_bits=obs_bits)
        if q16 is not None:
            self.set_action_noise(q16=q16)
        args = (self.h, int(T), self._slot_bits(slots, False, obs_bits), _ptr(actions), ctypes.byref(so), _ptr(obs),
                _ptr(vec), _stream(self.device))
        clean = args[:2] + (self._slot_bits(slots, not obs_bits, obs_bits),) + args[3:]
        fn = getattr(_lib.lib(), _policy_symbols(policy)[0])
        keep = (so, actions, obs, vec, out)
        state = [args]                  # the next call's arguments: `clean` once a call has stored the band

        entry = self._sparse_entry(T, obs) if sparse and slots and not obs_bits else None
        if entry is None:
            def launch():
                _lib.check(fn(*state[0]))
                state[0] = clean
                return keep[4], keep[2], keep[3]

            def invalidate():
                state[0] = args
            launch.invalidate = invalidate
            return launch

        fn_sparse = _lib.lib().mapf_rollout_sparse
        head = (self.h, SPARSE_POLICY[policy], int(T), args[3], args[4], args[5], args[6], _ptr(entry.shadow))
        stream, n = args[7], int(T)

        def launch_sparse():
            if obs._version != entry.version:       # torch wrote the buffer: the shadow says nothing now
                entry.valid = 0
                _lib.check(fn(*state[0]))
            else:
                _lib.check(fn_sparse(*head, entry.valid, stream))
                entry.valid = max(entry.valid, n)
            entry.version = obs._version
            state[0] = clean
            return keep[4], keep[2], keep[3]

        def invalidate_sparse():
            state[0] = args
            entry.valid = 0
        launch_sparse.invalidate = invalidate_sparse
        launch_sparse.sparse = entry
        return launch_sparse

    def _check_out(self, out):
        for k, t in out.items():
            ref = self.out[k]
            _check(t, ref.dtype, ref.numel(), self.device, k)
        return out

    def flush(self):
        """Run pending search work (BFS maps, next human paths) now, in its own launch."""
        _lib.check(_lib.lib().mapf_flush(self.h, _stream(self.device)))

    def release_captures(self):
        """Free the argument slots captured rollouts of this env took (mapf_release_captures):
        only after every hipGraph holding one has been destroyed."""
        _lib.check(_lib.lib().mapf_release_captures(self.h))

    def descent_actions(self, out=None):
        """The descent policy's actions for the current state (mapf_descent_actions; needs
        keep_bfs): int32 [B, N], every agent one step down its own BFS map, 0 at its goal."""
        out = self.actions if out is None else out
        _check(out, torch.int32, self.B * self.N, self.device, "actions")
        _lib.check(_lib.lib().mapf_descent_actions(self.h, _ptr(out), _stream(self.device)))
        return out

    def pibt_actions(self, out=None):
        """The PIBT policy's actions for the current state (mapf_pibt_actions; needs keep_bfs): int32
        [B, N], no two agents to one cell and no swap; updates the policy's ages."""
        out = self.actions if out is None else out
        _check(out, torch.int32, self.B * self.N, self.device, "actions")
        _lib.check(_lib.lib().mapf_pibt_actions(self.h, _ptr(out), _stream(self.device)))
        return out

    def set_action_noise(self, eps=None, *, q16=None):
        """Action noise of the picked policies' rollouts (mapf_set_action_noise; mapf.h has the rule): with
        probability eps, a float in [0, 1] (or q16=, the integer eps * 65536 in 0..65536), an agent plays
        the uniform random policy's action in place of the policy's pick, which stays the label the
        rollout's `actions` receive.  0, the default, is off.  It applies to "descent" and "pibt" rollouts
        (rollout, rollout_sparse, rollout_perf, launchers) and to noise_actions; "random" and "tape" ignore
        it.  Takes effect at the next launch; a captured launch keeps the value it was captured with.
        Resets leave it alone."""
        q = noise_q16(eps, q16)
        _lib.check(_lib.lib().mapf_set_action_noise(self.h, q))

    @property
    def action_noise(self):
        """The handle's action noise as q16 (mapf_get_action_noise)."""
        q = _lib.lib().mapf_get_action_noise(self.h)
        _lib.check(min(q, 0))
        return q

    def noise_actions(self, labels, out=None):
        """The actions played for `labels` (int32 [B, N]) under the handle's action noise at the current
        state's clocks (mapf_noise_actions): int32 [B, N]; out may be labels; a copy at noise 0."""
        _check(labels, torch.int32, self.B * self.N, self.device, "labels")
        if out is None:
            out = torch.empty_like(labels)
        _check(out, torch.int32, self.B * self.N, self.device, "played")
        _lib.check(_lib.lib().mapf_noise_actions(self.h, _ptr(labels), _ptr(out), _stream(self.device)))
        return out

    def set_pibt_human_weight(self, weight):
        """The PIBT policy's human weight w, an int in 0..16 (mapf_set_pibt_human_weight; mapf.h has the
        rule): a reachable target inside the human's safety radius costs w per level more.  0, the
        default, is the plain policy.  Takes effect at the next pibt_actions / rollout(T, "pibt");
        a captured launch keeps the weight it was captured with.  Resets leave it alone."""
        if isinstance(weight, bool) or not isinstance(weight, (int, np.integer)):
            raise TypeError(f"human weight: expected an int in 0..16, got {type(weight).__name__}")
        if not 0 <= int(weight) <= 16:
            raise ValueError(f"human weight must be in 0..16, got {int(weight)}")
        _lib.check(_lib.lib().mapf_set_pibt_human_weight(self.h, int(weight)))

    @property
    def pibt_human_weight(self):
        """The PIBT policy's human weight (mapf_get_pibt_human_weight)."""
        w = _lib.lib().mapf_get_pibt_human_weight(self.h)
        _lib.check(min(w, 0))
        return w

    def set_pibt_human_horizon(self, k):
        """The PIBT policy's human horizon K, an int in 1..8 (mapf_set_pibt_human_horizon; mapf.h has the
        rule): a target is priced against the human's next K predicted cells -- its next cell and the
        K - 1 that follow on its current path -- by the highest level among them.  1, the default,
        prices the next cell alone.  It has an effect only at a human weight above 0.  Takes effect at
        the next pibt_actions / rollout(T, "pibt"); a captured launch keeps the horizon it was captured
        with.  Resets leave it alone."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"human horizon: expected an int in 1..8, got {type(k).__name__}")
        if not 1 <= int(k) <= 8:
            raise ValueError(f"human horizon must be in 1..8, got {int(k)}")
        _lib.check(_lib.lib().mapf_set_pibt_human_horizon(self.h, int(k)))

    @property
    def pibt_human_horizon(self):
        """The PIBT policy's human horizon (mapf_get_pibt_human_horizon)."""
        k = _lib.lib().mapf_get_pibt_human_horizon(self.h)
        _lib.check(min(k, 0))
        return k

    def pibt_human_cells(self, out=None):
        """The human's predicted cells P_1..P_8 of the current state (mapf_pibt_human_cells), whatever
        the horizon: int32 [B, 8], each row | col << 16 as the state's cells are packed, -1 past the
        end of the human's current path."""
        if out is None:
            out = torch.empty((self.B, 8), dtype=torch.int32, device=self.device)
        _check(out, torch.int32, self.B * 8, self.device, "cells")
        _lib.check(_lib.lib().mapf_pibt_human_cells(self.h, _ptr(out), _stream(self.device)))
        return out

    def random_actions(self, out=None):
        out = self.actions if out is None else out
        _check(out, torch.int32, self.B * self.N, self.device, "actions")
        _lib.check(_lib.lib().mapf_random_actions(self.h, _ptr(out), _stream(self.device)))
        return out

    def bfs(self):
        d = torch.empty(self.B, self.N, self.H, self.W, dtype=torch.int16, device=self.device)
        _lib.check(_lib.lib().mapf_bfs(self.h, _ptr(d), _stream(self.device)))
        return d

    def render(self, envs=None, scale=20):
        """renderWorld (util.py:189-232) of the given envs (default all) on the device:
        uint8 RGB frames [n, H*scale, W*scale, 3] on this env's device."""
        idx = torch.arange(self.B, dtype=torch.int32) if envs is None else torch.as_tensor(envs, dtype=torch.int32)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.B):
            raise IndexError(f"env index out of range 0..{self.B - 1}")
        idx = idx.to(self.device).contiguous()
        out = torch.empty(idx.numel(), self.H * scale, self.W * scale, 3, dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().mapf_render(self.h, _ptr(idx), idx.numel(), int(scale), _ptr(out),
                                          _stream(self.device)))
        return out

    def counters(self):
        c = np.zeros(16, np.uint32)
        _lib.check(_lib.lib().mapf_get_counters(self.h, ctypes.c_void_p(c.ctypes.data), _stream(self.device)))
        return c

    def profile(self, reset=True):
        """Phase-cycle sums of the MAPF_STAMPS diagnostic build (zeros otherwise)."""
        c = np.zeros(16, np.uint64)
        _lib.check(_lib.lib().mapf_get_profile(self.h, ctypes.c_void_p(c.ctypes.data), int(reset),
                                               _stream(self.device)))
        return c

    def wave_profile(self, nwaves):
        """Diagnostic (stamps) build: per-wave phase cycles of the last step launch, uint64 [nwaves, 8]."""
        out = np.zeros((nwaves, 8), dtype=np.uint64)
        _lib.check(_lib.lib().mapf_get_wave_profile(self.h, out.ctypes.data_as(ctypes.c_void_p), nwaves,
                                                     _stream(self.device)))
        return out

    def timeline(self, nblocks):
        """Diagnostic (stamps) build: per-workgroup timeline of the last fused launch,
        uint64 [nblocks, 8] (realtime stamps 0-3 at 100 MHz, HW_ID, XCC_ID)."""
        out = np.zeros((nblocks, 8), dtype=np.uint64)
        _lib.check(_lib.lib().mapf_get_timeline(self.h, out.ctypes.data_as(ctypes.c_void_p), nblocks,
                                                 _stream(self.device)))
        return out

    def get_state(self):
        B, N, L = self.B, self.N, self.path_capacity
        st = dict(pos=np.zeros((B, N, 2), np.int32), goal=np.zeros((B, N, 2), np.int32),
                  last_action=np.zeros((B, N), np.int32), seq_cursor=np.zeros((B, N), np.int32),
                  human=np.zeros((B, 10), np.int32), human_path=np.zeros((B, L, 2), np.int32),
                  clock=np.zeros(B, np.uint32))
        s = _lib.State(*[st[n].ctypes.data for n, _ in _lib.State._fields_])
        _lib.check(_lib.lib().mapf_get_state(self.h, ctypes.byref(s), _stream(self.device)))
        return st

    def set_state(self, **kw):
        keep = {}
        s = _lib.State()
        for n, _ in _lib.State._fields_:
            if n in kw and kw[n] is not None:
                dt = np.uint32 if n == "clock" else np.int32
                a = np.ascontiguousarray(kw[n], dtype=dt)
                keep[n] = a
                setattr(s, n, a.ctypes.data)
        _lib.check(_lib.lib().mapf_set_state(self.h, ctypes.byref(s), _stream(self.device)))


def obs_words(C, F):
    """WPA: uint32 words of one agent's packed observation (ceil(C * F * F / 32))."""
    return (int(C) * int(F) * int(F) + 31) // 32


def is_packed_obs(obs, C, F):
    """A packed observation: int32 with last dimension WPA (floats are never int32)."""
    return isinstance(obs, torch.Tensor) and obs.dtype == torch.int32 and obs.dim() >= 1 and \
        obs.shape[-1] == obs_words(C, F)


def pack_obs(obs, C, F):
    """Host form of the packed format (mapf_obs_pack_host, the function the kernels store with):
    obs [..., C, F, F] float32 (a CPU tensor or array; non-zero packs as 1) -> int32 [..., WPA] on the CPU."""
    o = torch.as_tensor(obs, dtype=torch.float32, device="cpu").contiguous()
    C, F = int(C), int(F)
    if o.dim() < 3 or tuple(o.shape[-3:]) != (C, F, F):
        raise ValueError(f"pack_obs: shape {tuple(o.shape)}, expected [..., {C}, {F}, {F}]")
    lead = tuple(o.shape[:-3])
    n = o.numel() // (C * F * F)
    bits = torch.zeros(lead + (obs_words(C, F),), dtype=torch.int32)
    _lib.check(_lib.lib().mapf_obs_pack_host(_ptr(o), n, C, F, _ptr(bits)))
    return bits


def unpack_obs(bits, C, F, dtype=torch.float32, out=None):
    """bits int32 [..., WPA] -> [..., C, F, F] of 0 / 1 in `dtype` (float32 or float16).  On the GPU one
    HIP launch (mapf_unpack_obs; capturable, `out` may be any 4-byte aligned contiguous view); on the CPU
    torch bit operations (unpack_obs_host is the library's own host form)."""
    C, F = int(C), int(F)
    W, CFF = obs_words(C, F), C * F * F
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or bits.dim() < 1 or bits.shape[-1] != W:
        raise ValueError(f"unpack_obs: expected an int32 tensor [..., {W}]")
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("unpack_obs: dtype must be float32 or float16")
    lead = tuple(bits.shape[:-1])
    n = bits.numel() // W
    if out is None:
        out = torch.empty(lead + (C, F, F), dtype=dtype, device=bits.device)
    _check(out, dtype, n * CFF, bits.device, "out")
    if bits.device.type == "cpu":
        sh = torch.arange(32, dtype=torch.int32)
        b = ((bits.reshape(n, W, 1) >> sh) & 1).reshape(n, W * 32)[:, :CFF]
        out.view(-1)[:] = b.reshape(-1).to(dtype)
        return out
    b = _check(bits, torch.int32, n * W, bits.device, "bits")
    if out.data_ptr() % 4:
        raise ValueError("unpack_obs: out must be 4-byte aligned")
    _lib.check(_lib.lib().mapf_unpack_obs(_ptr(b), _ptr(out), n, C, F, int(dtype == torch.float16), _stream(bits.device)))
    return out


def unpack_obs_host(bits, C, F):
    """Host form (mapf_obs_unpack_host): int32 [..., WPA] on the CPU -> float32 [..., C, F, F]."""
    b = torch.as_tensor(bits, dtype=torch.int32, device="cpu").contiguous()
    C, F = int(C), int(F)
    if b.dim() < 1 or b.shape[-1] != obs_words(C, F):
        raise ValueError(f"unpack_obs_host: expected int32 [..., {obs_words(C, F)}]")
    out = torch.empty(tuple(b.shape[:-1]) + (C, F, F), dtype=torch.float32)
    _lib.check(_lib.lib().mapf_obs_unpack_host(_ptr(b), b.numel() // b.shape[-1], C, F, _ptr(out)))
    return out


def gae(rewards, values, last_values, gamma=0.95, lam=0.95):
    """runner.py:117-149 on device: rewards/values [T, ...] float32, last_values [...]."""
    T = rewards.shape[0]
    M = rewards[0].numel()
    dev = rewards.device
    if dev.type != "cuda":
        raise ValueError("gae: tensors must be on the GPU")
    _check(rewards, torch.float32, T * M, dev, "rewards")
    _check(values, torch.float32, T * M, dev, "values")
    _check(last_values, torch.float32, M, dev, "last_values")
    adv = torch.empty_like(rewards)
    ret = torch.empty_like(rewards)
    _lib.check(_lib.lib().mapf_gae(_ptr(rewards), _ptr(values), _ptr(last_values), _ptr(adv), _ptr(ret), T, M,
                                   gamma, lam, _stream(rewards.device)))
    return adv, ret


def normalize_advantages(returns, values, cost_returns, cost_values, lagrange=0.0, mix=False):
    """model.py:106-113 on device; returns (advantage, cost_advantage)."""
    dev, M = returns.device, returns.numel()
    if dev.type != "cuda":
        raise ValueError("normalize_advantages: tensors must be on the GPU")
    for name, t in (("returns", returns), ("values", values), ("cost_returns", cost_returns),
                    ("cost_values", cost_values)):
        _check(t, torch.float32, M, dev, name)
    adv = torch.empty_like(returns)
    cadv = torch.empty_like(returns)
    _lib.check(_lib.lib().mapf_normalize_advantages(
        _ptr(returns), _ptr(values), _ptr(cost_returns), _ptr(cost_values), _ptr(adv), _ptr(cadv),
        returns.numel(), float(lagrange), int(mix), _stream(returns.device)))
    return adv, cadv


def normalize_advantages_dlam(returns, values, cost_returns, cost_values, lam2, mix=False):
    """normalize_advantages with the multiplier in device memory: lam2 = float32 [2] on the GPU,
    {f32(lagrange), f32(lagrange + 1)} (mapf_normalize_advantages_dlam) -- capturable once and
    replayed with a new multiplier written into lam2."""
    dev, M = returns.device, returns.numel()
    for name, t in (("returns", returns), ("values", values), ("cost_returns", cost_returns),
                    ("cost_values", cost_values)):
        _check(t, torch.float32, M, dev, name)
    _check(lam2, torch.float32, 2, dev, "lam2")
    adv = torch.empty_like(returns)
    cadv = torch.empty_like(returns)
    _lib.check(_lib.lib().mapf_normalize_advantages_dlam(
        _ptr(returns), _ptr(values), _ptr(cost_returns), _ptr(cost_values), _ptr(adv), _ptr(cadv), M, _ptr(lam2),
        int(mix), _stream(dev)))
    return adv, cadv


def normalize_advantages_distributed(returns, values, cost_returns, cost_values, lagrange=0.0, mix=False, group=None,
                                     lam2=None):
    """normalize_advantages over a minibatch split across the ranks of torch.distributed: this
    rank's rows in, this rank's rows out, normalised with the GLOBAL mean and unbiased std
    (model.py:106-113 on the whole minibatch).  Two-pass fp64 moments on the device
    (mapf_advantage_moments), each pass all-reduced (2 small all-reduces), then
    mapf_normalize_advantages_stats.  lam2: the multiplier in device memory instead of
    `lagrange` (float32 [2] = {f32(lagrange), f32(lagrange + 1)}, as normalize_advantages_dlam;
    mapf_normalize_advantages_stats_dlam) -- Model.train's distributed device update."""
    if returns.device.type != "cuda":
        raise ValueError("normalize_advantages_distributed: tensors must be on the GPU")
    if lam2 is not None:
        _check(lam2, torch.float32, 2, returns.device, "lam2")
    stats = advantage_stats_distributed(returns, values, cost_returns, cost_values, group=group)
    return normalize_advantages_with_stats(returns, values, cost_returns, cost_values, stats, lagrange, mix, lam2)


def advantage_stats_distributed(returns, values, cost_returns, cost_values, group=None, out=None):
    """The GLOBAL advantage statistics of normalize_advantages_distributed: float64 [4] = {mean(r - v),
    mean(cr - cv), unbiased var(r - v), unbiased var(cr - cv)} over every rank's rows (two-pass fp64
    moments, each pass all-reduced).  out: a float64 [4] device tensor to write them into (the
    segmented captured update keeps them in a static buffer its graph reads)."""
    import torch.distributed as dist
    dev, M = returns.device, returns.numel()
    for name, t in (("returns", returns), ("values", values), ("cost_returns", cost_returns),
                    ("cost_values", cost_values)):
        _check(t, torch.float32, M, dev, name)
    st, L = _stream(dev), _lib.lib()
    ptrs = [_ptr(t) for t in (returns, values, cost_returns, cost_values)]
    buf = torch.zeros(3, dtype=torch.float64, device=dev)          # sum x, sum c, rows
    buf[2] = M
    _lib.check(L.mapf_advantage_moments(*ptrs, M, None, _ptr(buf), st))
    dist.all_reduce(buf, group=group)
    mean = (buf[:2] / buf[2]).contiguous()
    q = torch.zeros(2, dtype=torch.float64, device=dev)
    _lib.check(L.mapf_advantage_moments(*ptrs, M, _ptr(mean), _ptr(q), st))
    dist.all_reduce(q, group=group)
    stats = torch.cat([mean, q / (buf[2] - 1).clamp_min(1)])
    if out is None:
        return stats.contiguous()
    _check(out, torch.float64, 4, dev, "out")
    return out.copy_(stats)


def normalize_advantages_with_stats(returns, values, cost_returns, cost_values, stats, lagrange=0.0, mix=False,
                                    lam2=None):
    """model.py:106-113 with given statistics (advantage_stats_distributed's float64 [4]): this rank's
    rows normalised (mapf_normalize_advantages_stats[_dlam]); no collective, so capturable."""
    dev, M = returns.device, returns.numel()
    for name, t in (("returns", returns), ("values", values), ("cost_returns", cost_returns),
                    ("cost_values", cost_values)):
        _check(t, torch.float32, M, dev, name)
    _check(stats, torch.float64, 4, dev, "stats")
    if lam2 is not None:
        _check(lam2, torch.float32, 2, dev, "lam2")
    st, L = _stream(dev), _lib.lib()
    ptrs = [_ptr(t) for t in (returns, values, cost_returns, cost_values)]
    adv = torch.empty_like(returns)
    cadv = torch.empty_like(returns)
    if lam2 is None:
        _lib.check(L.mapf_normalize_advantages_stats(*ptrs, _ptr(stats), _ptr(adv), _ptr(cadv), M, float(lagrange),
                                                     int(mix), st))
    else:
        _lib.check(L.mapf_normalize_advantages_stats_dlam(*ptrs, _ptr(stats), _ptr(adv), _ptr(cadv), M, _ptr(lam2),
                                                          int(mix), st))
    return adv, cadv


def episode_sum(x):
    """OneEpPerformance.episodeReward-style sums (runner.py:95-96) of every env: x [T, B, N] float32
    on the GPU -> [B] float32, each step's numpy float32 np.sum over N accumulated in float32."""
    T, B, N = x.shape
    _check(x, torch.float32, T * B * N, x.device, "x")
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mapf_episode_sum(_ptr(x), T, B, N, _ptr(out), _stream(x.device)))
    return out


# the step outputs mapf_perf_accumulate reads (the others stay NULL)
PERF_INPUTS = ("status", "reward_total", "cost", "goals_reached", "shadow_goals", "constraints")


def perf_accumulate(out, perf=None, accumulate=False):
    """mapf_perf_accumulate (mapf.h): the episode metrics of every env from step outputs that already
    exist.  out: a dict of [T, B, N] (shadow_goals [T, B]) or one step's [B, N] ([B]) device tensors as the
    rollouts fill them; a missing key leaves its metrics at their previous value (or zero).  Returns perf,
    int32 [B, 8] (perf_dict), newly allocated if None; accumulate continues from what it holds."""
    ref = next((out[k] for k in PERF_INPUTS if k != "shadow_goals" and out.get(k) is not None), None)
    if ref is None:
        raise ValueError(f"out: none of {PERF_INPUTS} with an agent axis present")
    if ref.dim() not in (2, 3):
        raise ValueError(f"out: expected [T, B, N] or [B, N] tensors, got {tuple(ref.shape)}")
    T = ref.shape[0] if ref.dim() == 3 else 1
    B, N = ref.shape[-2], ref.shape[-1]
    so = _lib.StepOut()
    for k in PERF_INPUTS:
        t = out.get(k)
        if t is None:
            continue
        dtype = torch.int8 if k == "status" else (torch.int32 if k == "shadow_goals" else torch.float32)
        _check(t, dtype, T * B * (1 if k == "shadow_goals" else N), ref.device, k)
        setattr(so, k, t.data_ptr())
    if perf is None:
        if accumulate:
            raise ValueError("accumulate=True needs the perf to continue from")
        perf = torch.zeros(B, 8, dtype=torch.int32, device=ref.device)
    else:
        _check(perf, torch.int32, B * 8, ref.device, "perf")
    _lib.check(_lib.lib().mapf_perf_accumulate(ctypes.byref(so), T, B, N, _ptr(perf), 1 if accumulate else 0,
                                               _stream(ref.device)))
    return perf


def perf_dict(perf):
    """{METRIC_KEYS[i]: tensor [B]} of a perf tensor int32 [B, 8]: the two float metrics are the same bits
    viewed as float32 (reinterpreted, not converted), the six counts int32."""
    from .episodes import METRIC_KEYS
    if perf.dtype != torch.int32 or perf.dim() != 2 or perf.shape[1] != 8:
        raise ValueError(f"perf: expected int32 [B, 8], got {perf.dtype} {tuple(perf.shape)}")
    return {k: (perf[:, i].contiguous().view(torch.float32) if i < 2 else perf[:, i]) for i, k in enumerate(METRIC_KEYS)}


def sample_actions(ps, seed, step, out32=None, out64=None):
    """model.py:38-40 on device: ps [..., 5] float32 -> actions."""
    ps2 = ps.reshape(-1, ps.shape[-1])
    if ps2.dtype != torch.float32 or ps2.stride(1) != 1 or ps2.shape[-1] != 5 or ps2.device.type != "cuda":
        raise ValueError("sample_actions: ps must be float32 [..., 5] on the GPU with unit stride in the last dim")
    M = ps2.shape[0]
    if out32 is None and out64 is None:
        raise ValueError("sample_actions: give out32 and/or out64")
    if out32 is not None:
        _check(out32, torch.int32, M, ps2.device, "out32")
    if out64 is not None:
        _check(out64, torch.int64, M, ps2.device, "out64")
    _lib.check(_lib.lib().mapf_sample_actions(_ptr(ps2), ps2.stride(0), _ptr(out32), _ptr(out64), M, seed, step,
                                              _stream(ps.device)))
    return out32 if out32 is not None else out64


def minibatch_rows(n, seed, epoch, start, count, out=None, device=None):
    """Rows [start, start + count) of epoch `epoch`'s permutation of [0, n) (mapf_minibatch_rows:
    a keyed bijection computed element by element, no sort and no host indices): an int64 tensor
    [count].  out: the tensor to write (its device decides where); device="cpu" (or a CPU `out`)
    runs the host twin, the same function on the host -- no GPU needed."""
    n, start, count = int(n), int(start), int(count)
    if out is not None:
        device = out.device
    device = torch.device("cuda" if device is None else device)
    if out is None:
        out = torch.empty(max(count, 0), dtype=torch.int64, device=device)
    _check(out, torch.int64, max(count, 0), None, "out")
    seed, epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF
    if device.type == "cpu":
        _lib.check(_lib.lib().mapf_minibatch_rows_host(seed, epoch, n, start, count, _ptr(out)))
    else:
        _lib.check(_lib.lib().mapf_minibatch_rows(seed, epoch, n, start, count, _ptr(out), _stream(out.device)))
    return out


def gather_rows(srcs, T, B, rows, dsts):
    """dsts[a][j] = srcs[a][rows[j] % T, rows[j] // T] for up to 16 arrays in ONE launch
    (mapf_gather_rows): srcs t-major contiguous [T, B, ...] rollout buffers (views that start inside
    their storage included), rows int64 [M] on the device, ENV-MAJOR row ids in [0, B * T) (row r =
    env r // T, step r % T: runner.EnvMajorRows' order), dsts contiguous with M leading rows.  The
    rows are not range-checked on the device and not read back here: pass rows from minibatch_rows,
    or check explicit indices on the host first (DeviceTrainer / Model.train_rows do).  Capturable."""
    srcs, dsts = list(srcs), list(dsts)
    if len(srcs) != len(dsts) or not 1 <= len(srcs) <= _lib.GATHER_MAX:
        raise ValueError(f"gather_rows: {len(srcs)} sources and {len(dsts)} destinations (1..{_lib.GATHER_MAX} pairs)")
    T, B = int(T), int(B)
    if T < 1 or B < 1:
        raise ValueError("gather_rows: T and B must be >= 1")
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise ValueError("gather_rows: rows must be a tensor on the GPU")
    dev, M = rows.device, rows.numel()
    _check(rows, torch.int64, M, dev, "rows")
    if M < 1:
        raise ValueError("gather_rows: no rows")
    spec = _lib.GatherSpec(T=T, B=B, M=M, rows=rows.data_ptr(), count=len(srcs))
    for a, (src, dst) in enumerate(zip(srcs, dsts)):
        if not isinstance(src, torch.Tensor) or not isinstance(dst, torch.Tensor):
            raise TypeError(f"gather_rows: pair {a} is not a pair of tensors")
        if src.dtype != dst.dtype or src.device != dev or dst.device != dev:
            raise ValueError(f"gather_rows: pair {a}: {src.dtype} on {src.device} -> {dst.dtype} on {dst.device}, "
                             f"rows on {dev}")
        if src.dim() < 2 or tuple(src.shape[:2]) != (T, B) or not src.is_contiguous():
            raise ValueError(f"gather_rows: source {a} must be a contiguous [T={T}, B={B}, ...] buffer, got "
                             f"{tuple(src.shape)}")
        row = src[0, 0].numel()
        if dst.dim() < 1 or dst.shape[0] != M or dst.numel() != M * row or not dst.is_contiguous():
            raise ValueError(f"gather_rows: destination {a} must be contiguous with {M} rows of {row} elements, "
                             f"got {tuple(dst.shape)}")
        spec.arrays[a] = _lib.GatherArray(src.data_ptr(), dst.data_ptr(), row * src.element_size())
    _lib.check(_lib.lib().mapf_gather_rows(ctypes.byref(spec), _stream(dev)))
    return dsts


def sym_draw(seed, epoch, start, count, allowed=0xFF, out=None, device=None):
    """One grid symmetry g in 0..7 per element of the window [start, start + count) of the stream
    (seed, epoch), uniform over the set bits of the mask `allowed` (mapf_sym_draw: 0xFF the whole group,
    0x0F rotations only): a uint8 tensor [count].  Stateless like minibatch_rows, and like it
    device="cpu" (or a CPU `out`) runs the host twin."""
    start, count, allowed = int(start), int(count), int(allowed)
    if out is not None:
        device = out.device
    device = torch.device("cuda" if device is None else device)
    if out is None:
        out = torch.empty(max(count, 0), dtype=torch.uint8, device=device)
    _check(out, torch.uint8, max(count, 0), None, "out")
    if not 0 <= allowed <= 0xFFFFFFFF:
        raise ValueError(f"sym_draw: allowed {allowed:#x} is not an 8-bit mask")
    seed, epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF
    if device.type == "cpu":
        _lib.check(_lib.lib().mapf_sym_draw_host(seed, epoch, start, count, allowed, _ptr(out)))
    else:
        _lib.check(_lib.lib().mapf_sym_draw(seed, epoch, start, count, allowed, _ptr(out), _stream(out.device)))
    return out


def gather_rows_sym(srcs, T, B, rows, dsts, kinds, sym=None, geometry=None):
    """gather_rows with one grid symmetry per gathered row (mapf_gather_rows_sym, ONE launch): dsts[a][j]
    is row rows[j] of srcs[a] transformed by sym[j] as kinds[a] says -- "plain" (bytes), "obs" (float
    [N, C, F, F]), "obs_bits" (packed int32 [N, WPA] -> float [N, C, F, F], unpacked in the same pass),
    "vec" (float [N, 4]), "action32" / "action64" (int [N]), "cols" (float [N, 5]: train_valid, ps).
    sym: uint8 [M] on the device, g in 0..7 (sym_draw), or None for the identity; geometry = (N, C, F).
    With sym=None the destinations hold gather_rows' bytes (unpack_obs' for "obs_bits").  Capturable."""
    srcs, dsts, kinds = list(srcs), list(dsts), list(kinds)
    if not (len(srcs) == len(dsts) == len(kinds)) or not 1 <= len(srcs) <= _lib.GATHER_MAX:
        raise ValueError(f"gather_rows_sym: {len(srcs)} sources, {len(dsts)} destinations and {len(kinds)} kinds "
                         f"(1..{_lib.GATHER_MAX} triples)")
    if geometry is None or len(geometry) != 3:
        raise ValueError("gather_rows_sym: geometry=(N, C, F) is required")
    N, C, F = (int(x) for x in geometry)
    T, B = int(T), int(B)
    if T < 1 or B < 1:
        raise ValueError("gather_rows_sym: T and B must be >= 1")
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise ValueError("gather_rows_sym: rows must be a tensor on the GPU")
    dev, M = rows.device, rows.numel()
    _check(rows, torch.int64, M, dev, "rows")
    if M < 1:
        raise ValueError("gather_rows_sym: no rows")
    if sym is not None:
        _check(sym, torch.uint8, M, dev, "sym")
    spec = _lib.GatherSymSpec(T=T, B=B, M=M, rows=rows.data_ptr(), sym=None if sym is None else sym.data_ptr(),
                              N=N, C=C, F=F, count=len(srcs))
    for a, (src, dst, kind) in enumerate(zip(srcs, dsts, kinds)):
        if kind not in _lib.GATHER_KINDS:
            raise ValueError(f"gather_rows_sym: kind {kind!r} of array {a} is not one of {sorted(_lib.GATHER_KINDS)}")
        if not isinstance(src, torch.Tensor) or not isinstance(dst, torch.Tensor):
            raise TypeError(f"gather_rows_sym: triple {a} holds no pair of tensors")
        want = {"obs": (torch.float32, torch.float32), "obs_bits": (torch.int32, torch.float32),
                "vec": (torch.float32, torch.float32), "action32": (torch.int32, torch.int32),
                "action64": (torch.int64, torch.int64), "cols": (torch.float32, torch.float32)}.get(kind, (src.dtype, src.dtype))
        if (src.dtype, dst.dtype) != want or src.device != dev or dst.device != dev:
            raise ValueError(f"gather_rows_sym: array {a} ({kind}): {src.dtype} on {src.device} -> {dst.dtype} on "
                             f"{dst.device}, rows on {dev}")
        if src.dim() < 2 or tuple(src.shape[:2]) != (T, B) or not src.is_contiguous():
            raise ValueError(f"gather_rows_sym: source {a} must be a contiguous [T={T}, B={B}, ...] buffer, got "
                             f"{tuple(src.shape)}")
        row = src[0, 0].numel()
        drow = N * C * F * F if kind == "obs_bits" else row
        if dst.dim() < 1 or dst.shape[0] != M or dst.numel() != M * drow or not dst.is_contiguous():
            raise ValueError(f"gather_rows_sym: destination {a} must be contiguous with {M} rows of {drow} elements, "
                             f"got {tuple(dst.shape)}")
        spec.arrays[a] = _lib.GatherSymArray(src.data_ptr(), dst.data_ptr(), row * src.element_size(),
                                             drow * dst.element_size(), _lib.GATHER_KINDS[kind], 0)
    _lib.check(_lib.lib().mapf_gather_rows_sym(ctypes.byref(spec), _stream(dev)))
    return dsts


def _sym_action(g, a):
    """include/mapf.h, "Grid symmetries": the mirror swaps moves 1 and 3, a quarter turn takes move a to a - 1
    (1 to 4); 0 stays (csrc/mapf_sym.h: sym_action is the rule, tests/test_sym_cpu.py compares)"""
    if a == 0:
        return 0
    if g & 4 and a & 1:
        a = 4 - a
    return 1 + ((a - 1 - (g & 3)) & 3)


_SYM_ACTION = [[_sym_action(g, a) for a in range(5)] for g in range(8)]


def sym_apply(obs, vec, actions, cols, g):
    """The grid symmetries in plain torch, for models off the GPU and as the reference of the kernels:
    (obs [M, ..., F, F], vec [M, ..., 4], actions [M, ...] of any int dtype, cols [M, ..., 5]) transformed by
    g -- one int for every row, or M of them (a sequence or tensor).  Any of the four may be None; numpy
    arrays come back as numpy arrays.  Bit-equal to the host twins (mapf_sym_*_host)."""
    import numpy as np
    first = next((x for x in (obs, vec, actions, cols) if x is not None), None)
    if first is None:
        return None, None, None, None
    M = first.shape[0]
    gs = torch.as_tensor(g).reshape(-1).to("cpu", torch.int64) & 7
    if gs.numel() == 1:
        gs = gs.expand(M)
    if gs.numel() != M:
        raise ValueError(f"sym_apply: {gs.numel()} symmetries for {M} rows")
    outs = []
    for what, x in (("obs", obs), ("vec", vec), ("actions", actions), ("cols", cols)):
        if x is None:
            outs.append(None)
            continue
        was_numpy = isinstance(x, np.ndarray)
        t = torch.from_numpy(x) if was_numpy else x
        if t.shape[0] != M:
            raise ValueError(f"sym_apply: {what} has {t.shape[0]} rows, expected {M}")
        out = t.clone()
        for gv in torch.unique(gs).tolist():
            if gv == 0:
                continue
            sel = (gs == gv).nonzero().reshape(-1).to(t.device)
            y = t[sel]
            if what == "obs":
                y = torch.rot90(torch.flip(y, (-1,)) if gv & 4 else y, gv & 3, (-2, -1))
            elif what == "vec":
                a, b = y[..., 0], y[..., 1]
                if gv & 4:
                    b = 0.0 - b
                for _ in range(gv & 3):
                    a, b = 0.0 - b, a
                y = torch.stack((a, b, y[..., 2], y[..., 3]), dim=-1)
            elif what == "actions":
                table = torch.tensor(_SYM_ACTION[gv], dtype=y.dtype, device=y.device)
                inside = (y >= 0) & (y <= 4)
                y = torch.where(inside, table[y.clamp(0, 4).long()], y)
            else:
                perm = torch.tensor(_SYM_ACTION[gv], device=y.device)
                z = torch.empty_like(y)
                z[..., perm] = y
                y = z
            out[sel] = y
        outs.append(out.numpy() if was_numpy else out)
    return tuple(outs)
