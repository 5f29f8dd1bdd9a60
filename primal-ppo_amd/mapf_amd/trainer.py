"""DeviceTrainer: PPO epochs over ALL B * T rows of a DeviceRunner rollout.

The reference's driver (driver.py:123-134) shuffles `np.arange(N_STEPS)` on the host and indexes
twelve arrays with it per minibatch -- over this engine's env-major rows that is env 0's rollout
only, T of the B * T rows.  Here every epoch walks one permutation of all B * T rows, computed on
the device (env.minibatch_rows: a keyed bijection, no sort, no host indices), and each minibatch
is gathered from the rollout buffers into the captured update's static inputs by one HIP launch
(Model.train_rows -> _DeviceUpdate.load_rows -> env.gather_rows).

Rows are ENV-MAJOR, as everywhere in runner.py: row r = env r // T, step r % T.

The minibatch shape is static (the update is captured per shape), so an epoch trains
K = (B * T) // minibatch minibatches and leaves the (B * T) % minibatch last rows of its
permutation out; the epoch counter moves on across update() calls, so no two epochs share a
permutation and other rows are left out each time.

imitate(source) walks the same kind of epochs over a source of demonstrations (imitation.DemoRunner,
or a DeviceRunner built with expert=) through Model.imitate_rows, and fit(n, demo=, demonstration_prob=)
draws per rollout which of the two it is (TrainingParameters.DEMONSTRATION_PROB).

augment=MASK (off by default) draws one of the square's eight symmetries per minibatch row
(env.sym_draw, keyed by the trainer's seed and epoch counter) and passes it down as sym=: the gather
then transforms observation, vec, action and the per-action columns together (env.gather_rows_sym).

Several ranks: every rank must hold the same B and T (Model's distributed update needs equal
minibatch counts on every rank); each rank shuffles its own rollout.
"""
import numpy as np
import torch

from .config import TrainingParameters
from .env import minibatch_rows, sym_draw


class DeviceTrainer:
    def __init__(self, runner, model, minibatch=None, n_epochs=None, seed=0, augment=None):
        self.runner, self.model = runner, model
        self.minibatch = TrainingParameters.MINIBATCH_SIZE if minibatch is None else int(minibatch)
        self.n_epochs = TrainingParameters.N_EPOCHS if n_epochs is None else int(n_epochs)
        self.seed = int(seed)
        self.epoch_counter = 0
        self.n = runner.T * runner.env.B
        if not 1 <= self.minibatch <= self.n:
            raise ValueError(f"minibatch {self.minibatch} for a rollout of {self.n} rows")
        self.rows = None                        # the minibatch's row ids: one device tensor, reused
        # grid-symmetry augmentation: the mask of allowed symmetries (env.sym_draw: 0xFF the whole group,
        # 0x0F rotations only); None or 0x01 (identity only) = off, nothing is drawn and nothing changes
        self.augment = None if augment is None or int(augment) == 0x01 else int(augment)
        if self.augment is not None and not 1 <= self.augment <= 0xFF:
            raise ValueError(f"augment {augment!r} is not a mask of the eight symmetries (1..0xFF)")
        self.sym = None                         # the minibatch's symmetries: one device tensor, reused

    def _sym_arg(self, k, M):
        """the sym= argument of minibatch k's train_rows / imitate_rows: nothing with augmentation off (a
        model without the argument still serves), else window [k * M, (k + 1) * M) of the epoch's draws"""
        if self.augment is None:
            return {}
        if self.sym is None:
            self.sym = torch.empty(M, dtype=torch.uint8, device=self.rows.device)
        return {"sym": sym_draw(self.seed, self.epoch_counter, k * M, M, self.augment, out=self.sym)}

    def minibatches_per_epoch(self):
        return self.n // self.minibatch

    def update(self, performance):
        """N_EPOCHS epochs over the runner's last rollout: per epoch (B * T) // minibatch updates, minibatch
        k on rows [k * M, (k + 1) * M) of that epoch's permutation.  performance: the rollout's
        OneEpPerformance (its episodeCostReward feeds the Lagrangian, model.py:180).  Returns the
        per-minibatch stats in order -- driver.py's mb_loss."""
        M, dev = self.minibatch, self.runner.env.device
        on_gpu = self.model.device.type == "cuda"
        if self.rows is None:
            self.rows = torch.empty(M, dtype=torch.int64, device=dev if on_gpu else "cpu")
        mb_loss = []
        for _ in range(self.n_epochs):
            for k in range(self.minibatches_per_epoch()):
                minibatch_rows(self.n, self.seed, self.epoch_counter, k * M, M, out=self.rows)
                mb_loss.append(self.model.train_rows(self.runner, self.rows, performance.episodeCostReward,
                                                     checked=True, **self._sym_arg(k, M)))
            self.epoch_counter += 1
        return mb_loss

    def imitate(self, source, n_epochs=1):
        """n_epochs epochs of behaviour cloning over source's last rollout (imitation.DemoRunner, or a
        DeviceRunner built with expert=): per epoch (source.T * B) // minibatch updates, minibatch k on rows
        [k * M, (k + 1) * M) of that epoch's permutation, through Model.imitate_rows.  The epoch counter is
        update()'s, so PPO and imitation epochs never share a permutation.  Returns the per-minibatch stats
        (loss, grad norm, agreement with the expert, the expert action's mean probability)."""
        M = self.minibatch
        n = source.T * source.env.B
        if not 1 <= M <= n:
            raise ValueError(f"minibatch {M} for a rollout of {n} rows")
        on_gpu = self.model.device.type == "cuda"
        if self.rows is None:
            self.rows = torch.empty(M, dtype=torch.int64, device=source.env.device if on_gpu else "cpu")
        mb_loss = []
        for _ in range(int(n_epochs)):
            for k in range(n // M):
                minibatch_rows(n, self.seed, self.epoch_counter, k * M, M, out=self.rows)
                mb_loss.append(self.model.imitate_rows(source, self.rows, checked=True, **self._sym_arg(k, M)))
            self.epoch_counter += 1
        return mb_loss

    def fit(self, n_rollouts, demo=None, demonstration_prob=None):
        """n_rollouts times: runner.run(), then update() on it.  The trained weights are handed to the
        runner only when it acts with another Model object than the one trained.  Returns the list of
        (performance, mb_loss) per rollout.
        demo: a source of demonstrations (imitation.DemoRunner).  Each rollout index is then an imitation
        rollout -- demo.run(), then imitate(demo) -- with probability demonstration_prob (default
        TrainingParameters.DEMONSTRATION_PROB = 0: never, driver.py's setting), drawn from a host generator
        seeded with the trainer's seed; otherwise the PPO rollout.  With demo given, the entries are
        (kind, performance, mb_loss), kind "ppo" or "imitation" (an imitation entry's performance is
        demo.run()'s per-env counters)."""
        if demo is None:
            if demonstration_prob:
                raise ValueError("demonstration_prob needs a source of demonstrations: demo=...")
            prob, draw = 0.0, None
        else:
            prob = float(TrainingParameters.DEMONSTRATION_PROB if demonstration_prob is None else demonstration_prob)
            if not 0.0 <= prob <= 1.0:
                raise ValueError(f"demonstration_prob {prob} outside [0, 1]")
            if getattr(self, "_demo_rng", None) is None:
                self._demo_rng = np.random.default_rng([self.seed & 0xFFFFFFFF, 0x1A17A7E])
            draw = self._demo_rng
        out = []
        for _ in range(int(n_rollouts)):
            if prob > 0.0 and draw.random() < prob:
                performance = demo.run()
                out.append(("imitation", performance, self.imitate(demo)))
                continue
            weights = None if self.runner.model is self.model else self.model.network.state_dict()
            _, performance = self.runner.run(weights)
            mb_loss = self.update(performance)
            out.append((performance, mb_loss) if demo is None else ("ppo", performance, mb_loss))
        return out
