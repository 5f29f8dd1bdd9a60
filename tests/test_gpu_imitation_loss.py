"""GPU tests of the fused imitation loss (csrc/mapf_imitation.hip, mapf_imitation_loss): its value,
its two terms and its gradient against autograd through the reference's own expression
(F.cross_entropy under autocast, model.py:221-222) and a torch restatement of the terms; fp32 and fp16
logits, int32 and int64 actions, one row to more rows than one pass of the workgroup holds, and the
rows where a softmax goes wrong first: a 120-wide spread, the fp16 extremes, ties."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (24, 5), (1025, 5), (12000, 5), (64, 3)]      # 1025: one row past the 1024 threads' first pass


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _inputs(R, A, dtype, act_dtype):
    g = torch.Generator(device="cuda").manual_seed(R * 31 + A)
    logits = (torch.randn(R, A, device="cuda", generator=g) * 3).to(dtype)
    action = torch.randint(0, A, (R,), device="cuda", generator=g)
    special = []
    if A == 5:
        special.append(([60.0, -60.0, 0.0, 0.0, 0.0], 1))           # exp(-120): the expert's action nearly impossible
        special.append(([1.5] * 5, 0))                              # all equal: argmax is index 0, and it agrees
        special.append(([1.5] * 5, 3))                              # all equal, the expert elsewhere: no agreement
        if dtype == torch.float16:
            special.append(([65504.0, -65504.0, 0.0, -65504.0, 65504.0], 4))      # the fp16 extremes, a tie at the top
            special.append(([65504.0, -65504.0, 0.0, -65504.0, 65504.0], 1))
    for k, (row, a) in enumerate(special[:R]):
        logits[k] = torch.tensor(row, device="cuda").to(dtype)
        action[k] = a
    return logits, action.to(act_dtype)


def torch_terms(logits, action):
    """agreement (argmax = the smallest index among the maxima) and the expert action's mean probability"""
    l32, a = logits.detach().float(), action.long()
    top = l32.max(dim=-1, keepdim=True).values
    A = l32.shape[-1]
    first = torch.where(l32 == top, torch.arange(A, device=l32.device), A).min(dim=-1).values
    p = torch.softmax(l32, -1).gather(-1, a[:, None]).squeeze(-1)
    return torch.stack([(first == a).float().mean(), p.mean()])


@pytest.mark.parametrize("act_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("R,A", SHAPES)
def test_fused_loss_terms_and_gradient_vs_autograd(R, A, dtype, act_dtype):
    from mapf_amd.model import _FusedImitationLoss
    logits, action = _inputs(R, A, dtype, act_dtype)
    a = logits.clone().requires_grad_(True)
    b = logits.clone().requires_grad_(True)
    with torch.autocast(device_type="cuda"):           # as in Model.imitation_train: cross_entropy autocasts to fp32
        ref_loss = F.cross_entropy(a, action.long())
    ref_loss.backward()
    loss, terms = _FusedImitationLoss.apply(b, action)
    assert not terms.requires_grad and loss.dtype == torch.float32
    (loss * 3.0).backward()                             # an upstream scale, like GradScaler's
    torch.testing.assert_close(loss, ref_loss.detach().float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(terms, torch_terms(logits, action), rtol=1e-5, atol=1e-6)
    assert b.grad.dtype == dtype and b.grad.shape == b.shape
    tol = 2e-3 if dtype == torch.float16 else 1e-5
    torch.testing.assert_close(b.grad.float(), 3.0 * a.grad.float(), rtol=tol, atol=tol * 1e-3)


def test_agreement_counts_the_first_maximum():
    from mapf_amd.model import _FusedImitationLoss
    logits = torch.tensor([[2.0, 2.0, 2.0, 2.0, 2.0], [2.0, 2.0, 2.0, 2.0, 2.0], [0.0, 7.0, 7.0, 1.0, 7.0],
                           [0.0, 7.0, 7.0, 1.0, 7.0]], device="cuda")
    action = torch.tensor([0, 4, 1, 2], dtype=torch.int32, device="cuda")
    _, terms = _FusedImitationLoss.apply(logits, action)
    assert terms[0].item() == 0.5


def test_leading_shape_and_the_c_call_leave_their_neighbours_alone():
    """[rows, agents, A] logits as the network hands them over; the raw call writes loss[1], terms[2] and
    grad[R][A] and nothing after them."""
    from mapf_amd import _lib
    from mapf_amd.model import _FusedImitationLoss
    g = torch.Generator(device="cuda").manual_seed(4)
    logits = torch.randn(7, 8, 5, device="cuda", generator=g).half().requires_grad_(True)
    action = torch.randint(0, 5, (7, 8), device="cuda", generator=g, dtype=torch.int32)
    loss, _ = _FusedImitationLoss.apply(logits, action)
    loss.backward()
    with torch.autocast(device_type="cuda"):
        ref = F.cross_entropy(logits.detach().swapaxes(1, 2), action.long())
    torch.testing.assert_close(loss.detach(), ref, rtol=1e-5, atol=1e-6)
    assert logits.grad.shape == (7, 8, 5)
    R, A = 56, 5
    out = torch.full((3 + 1 + R * A + 3,), float("nan"), device="cuda")
    _lib.call("mapf_imitation_loss", logits.detach().reshape(R, A).contiguous(), 1, action.reshape(R).contiguous(), 0,
              R, A, out[0:1], out[1:3], out[4:4 + R * A])
    assert torch.isfinite(out[:3]).all() and torch.isnan(out[3]) and torch.isfinite(out[4:4 + R * A]).all()
    assert torch.isnan(out[4 + R * A:]).all()
    torch.testing.assert_close(out[0], ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("bad", [5, -1, 2 ** 40])
def test_out_of_range_action_poisons_the_loss(bad):
    from mapf_amd.model import _FusedImitationLoss
    logits = torch.randn(9, 5, device="cuda")
    action = torch.randint(0, 5, (9,), device="cuda")
    action[4] = bad
    loss, terms = _FusedImitationLoss.apply(logits, action)
    assert torch.isnan(loss) and torch.isfinite(terms).all()
    if abs(bad) < 2 ** 31:
        loss, _ = _FusedImitationLoss.apply(logits, action.int())
        assert torch.isnan(loss)


def test_one_launch_is_capturable_and_deterministic():
    from mapf_amd.model import _FusedImitationLoss
    logits, action = _inputs(12000, 5, torch.float16, torch.int32)
    first = [t.clone() for t in _FusedImitationLoss.apply(logits, action)]
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _FusedImitationLoss.apply(logits, action)                   # allocator warm-up on the capture stream
        with torch.cuda.graph(g, stream=s):
            loss, terms = _FusedImitationLoss.apply(logits, action)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        loss.fill_(float("nan"))
        g.replay()
        assert torch.equal(loss, first[0]) and torch.equal(terms, first[1])       # bitwise: a fixed-order reduction
