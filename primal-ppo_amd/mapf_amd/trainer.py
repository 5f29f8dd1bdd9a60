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

Several ranks: every rank must hold the same B and T (Model's distributed update needs equal
minibatch counts on every rank); each rank shuffles its own rollout.
"""
import torch

from .config import TrainingParameters
from .env import minibatch_rows


class DeviceTrainer:
    def __init__(self, runner, model, minibatch=None, n_epochs=None, seed=0):
        self.runner, self.model = runner, model
        self.minibatch = TrainingParameters.MINIBATCH_SIZE if minibatch is None else int(minibatch)
        self.n_epochs = TrainingParameters.N_EPOCHS if n_epochs is None else int(n_epochs)
        self.seed = int(seed)
        self.epoch_counter = 0
        self.n = runner.T * runner.env.B
        if not 1 <= self.minibatch <= self.n:
            raise ValueError(f"minibatch {self.minibatch} for a rollout of {self.n} rows")
        self.rows = None                        # the minibatch's row ids: one device tensor, reused

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
                                                     checked=True))
            self.epoch_counter += 1
        return mb_loss

    def fit(self, n_rollouts):
        """n_rollouts times: runner.run(), then update() on it.  The trained weights are handed to the
        runner only when it acts with another Model object than the one trained.  Returns the list of
        (performance, mb_loss) per rollout."""
        out = []
        for _ in range(int(n_rollouts)):
            weights = None if self.runner.model is self.model else self.model.network.state_dict()
            _, performance = self.runner.run(weights)
            out.append((performance, self.update(performance)))
        return out
