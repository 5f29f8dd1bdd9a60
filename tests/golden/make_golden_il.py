"""Generate tests/golden/g9_imitation.npz from the reference's own Model.imitation_train.

Run where the reference exists (make_golden.py's REF), from the repository root:

    python tests/golden/make_golden_il.py

Like make_golden.py this drives the reference's classes and records inputs and outputs; the
fixture is data only.  One behaviour-cloning update (model.py:205-231) on CPU, fp32, eval mode
(dropout off): 16 rows x 8 agents, FOV 9, 6 channels, inputs and weights from tests/imitation_ref.py.
Stored: the inputs (obs bit-packed), the logits before the update, the loss, the grad norm, and for
every parameter that received a gradient its L2 norm and first 1,024 elements, read after
imitation_train (so unscaled and clipped).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from make_golden import OUT, import_reference, set_params  # noqa: E402
import imitation_ref as R  # noqa: E402

MIN_VISIBLE = 1e-3          # every parameter's gradient norm against the largest (token_wA: exactly 0)


def g9_imitation():
    import_reference()
    set_params(R.AGENTS, R.FOV)
    import torch
    import model as model_mod
    torch.manual_seed(0)
    m = model_mod.Model(0, torch.device("cpu"), global_model=True, numChannel=R.CHANNELS)
    R.load_recipe(m.network)
    m.network.eval()
    obs, vec, action = R.inputs()
    hidden = np.zeros((R.ROWS, 2, R.AGENTS, 512), np.float32)
    with torch.no_grad():
        logits = m.network(torch.from_numpy(obs), torch.from_numpy(vec), None)[5].numpy()
    loss, grad_norm = m.imitation_train(obs, vec, action, hidden)
    grads = R.grad_slices(m.network)
    names = sorted(grads)
    norms = np.array([grads[n][0] for n in names])
    no_grad = sorted(n for n, p in m.network.named_parameters() if p.grad is None)
    ratio = norms / norms.max()
    for n, r in zip(names, ratio):
        assert (n == "token_wA" and r == 0.0) or r >= MIN_VISIBLE, (n, r)
    out = dict(obs_packed=np.packbits(obs.astype(np.uint8)), obs_shape=np.array(obs.shape), vec=vec, action=action,
               logits=logits, loss=np.float32(loss), grad_norm=np.float32(grad_norm), names=np.array(names),
               no_grad=np.array(no_grad), norms=norms.astype(np.float64))
    for n in names:
        out[R.grad_key(n)] = grads[n][1]
    np.savez_compressed(os.path.join(OUT, "g9_imitation.npz"), **out)
    k = int(np.argmin(np.where(ratio > 0, ratio, np.inf)))
    print(f"g9_imitation: loss {float(loss):.6f} grad norm {float(grad_norm):.5f}; {len(names)} gradients, "
          f"smallest visible {names[k]} at {ratio[k]:.2e} of the largest; no gradient: {no_grad}")


if __name__ == "__main__":
    g9_imitation()
