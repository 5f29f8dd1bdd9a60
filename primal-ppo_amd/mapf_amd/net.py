"""SCRIMPNet policy/value network, state_dict-compatible with the reference.

Architecture and parameter names follow net.py:38-155 and transformer.py:1-100
of the reference so that a reference checkpoint (`torch.save({"model": ...})`,
driver.py:182-193) loads with `load_state_dict` unchanged:

  obs [.., C, F, F] -> 3x conv3x3(128) -> maxpool -> 3x conv2x2(256) -> maxpool
  -> conv3x3(500) -> flatten ++ fc(vector 4 -> 12) -> 512 -> residual MLP
  -> 16-token tokeniser + cls token + positional embedding
  -> 2 pre-norm transformer blocks (16 heads, MLP 512, GELU, dropout 0.2)
  -> cls -> nn_same applied twice -> policy(5) / value / cost value / blocking

The tokeniser keeps the reference's exact arithmetic: its einsum
'bij,zjk->bik' SUMS over the 8 token matrices and its softmax runs over a
length-1 axis, so every token equals the summed-V projection (kept literally).
Runs under torch autocast like the reference (net.py:101).

This module is the architecture and its dispatch only: the training forward on the GPU (train_ops.hip_training)
takes the HIP autograd Functions of train_ops.py, the no-grad forward on the GPU is acting.forward_fused.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import acting
from .config import EnvParameters, NetParameters
from .train_ops import (_OWN_CONV, _BiasReLU, _BiasReLUPool, _CastParams, _DropResLN, _GeluDropout, _HipAttention,
                        _HipConv, _HipLayerNorm, _QKVFirst, _SplitKLinear, _TokensLN, _drop_p, _train_linear,
                        hip_training)


def _xavier_like(module):
    """weights_init (net.py:18-35): uniform(+-sqrt(6/(fan_in+fan_out))), zero bias."""
    name = module.__class__.__name__
    if name.find("Conv") != -1:
        shape = list(module.weight.data.size())
        fan_in = np.prod(shape[1:4])
        fan_out = np.prod(shape[2:4]) * shape[0]
        bound = math.sqrt(6.0 / (fan_in + fan_out))
        module.weight.data.uniform_(-bound, bound)
        module.bias.data.fill_(0)
    elif name.find("Linear") != -1:
        fan_out, fan_in = module.weight.data.size()
        bound = math.sqrt(6.0 / (fan_in + fan_out))
        module.weight.data.uniform_(-bound, bound)
        if module.bias is not None:
            module.bias.data.fill_(0)


class _PreNorm(nn.Module):
    """Residual(LayerNormalize(dim, fn)) of transformer.py:7-24 (state_dict path `.fn.norm` / `.fn.fn`)."""

    def __init__(self, dim, fn):
        super().__init__()
        self.fn = nn.Module()
        self.fn.norm = nn.LayerNorm(dim)
        self.fn.fn = fn

    def _norm(self, x):
        """(LayerNorm(x), the residual x): on the GPU training path one _HipLayerNorm whose backward
        also takes the residual's gradient"""
        n = self.fn.norm
        if hip_training(x) and x.dtype == torch.float32 and x.shape[-1] == 512 and n.elementwise_affine:
            return _HipLayerNorm.apply(x, n.weight, n.bias, n.eps)
        return n(x), x

    def forward(self, x):
        z, res = self._norm(x)
        return self.fn.fn(z) + res

    def forward_first(self, x):
        """Token 0 of forward(x) only (x: [b, n, d] -> [b, 1, d])."""
        z, res = self._norm(x)
        return self.fn.fn.forward_first(z) + res[:, :1]


class _SelfAttention(nn.Module):
    """transformer.py:48-85: fused qkv projection, softmax(q k^T / sqrt(dim)) v, output projection.
    Note the reference scales by dim ** -0.5 (the model width), not the head width.
    The attention itself is one fused scaled_dot_product_attention call (no dropout on
    the attention weights, as in the reference): 17 tokens x 16 heads x 32 per agent
    as batched GEMMs would be ~500k tiny matrix products per layer."""

    def __init__(self, dim, heads, dropout):
        super().__init__()
        self.heads = heads
        self.scale = dim ** -0.5
        self.to_qkv = nn.Linear(dim, dim * 3, bias=True)
        nn.init.xavier_uniform_(self.to_qkv.weight)
        nn.init.zeros_(self.to_qkv.bias)
        self.nn1 = nn.Linear(dim, dim)
        nn.init.xavier_uniform_(self.nn1.weight)
        nn.init.zeros_(self.nn1.bias)
        self.do1 = nn.Dropout(dropout)

    hip_attention = True               # the training forward's attention on _HipAttention (GPU, fp16)

    def _hip(self, x, t):
        return (self.hip_attention and hip_training(x) and t.dtype == torch.float16 and self.heads == 16 and
                x.shape[-1] == 512 and x.shape[1] <= 32)

    def forward(self, x):
        return self.do1(self.forward_core(x))

    def forward_core(self, x):
        """forward(x) before its dropout (the fused training residual applies it)"""
        b, n, d = x.shape
        h = self.heads
        qkv = _train_linear(x, self.to_qkv.weight, self.to_qkv.bias)
        if self._hip(x, qkv):
            att = _HipAttention.apply(qkv.contiguous(), qkv.contiguous(), n, 0, d, 2 * d, self.scale)
            return _train_linear(att, self.nn1.weight, self.nn1.bias)
        qkv = qkv.view(b, n, 3, h, d // h).permute(2, 0, 3, 1, 4)   # 3, b, h, n, dh
        q, k, v = qkv[0], qkv[1], qkv[2]
        out = F.scaled_dot_product_attention(q, k, v, scale=self.scale).transpose(1, 2).reshape(b, n, d)
        return self.nn1(out)

    def forward_first(self, x):
        """Token 0 of forward(x) only: keys and values of every token, the query of token 0."""
        return self.do1(self.forward_first_core(x))

    def forward_first_core(self, x):
        b, n, d = x.shape
        h = self.heads
        w, bias = self.to_qkv.weight, self.to_qkv.bias
        # x[:, 0] is a 2-D strided view: one GEMM with lda = n*d ([b, 1, d] would run as a slow bmm)
        # the q / kv projections and their backward as one _QKVFirst
        if (hip_training(x) and x.dtype == w.dtype == bias.dtype == torch.float16 and x.is_contiguous() and
                d % 8 == 0 and w.requires_grad and b * n >= _SplitKLinear.MIN_ROWS):
            q, kv = _QKVFirst.apply(x, w, bias)
        else:
            q = _train_linear(x[:, 0], w[:d], bias[:d])
            kv = _train_linear(x, w[d:], bias[d:])
        if self._hip(x, q):
            att = _HipAttention.apply(q.contiguous(), kv.contiguous(), 1, 0, 0, d, self.scale)
            return _train_linear(att.reshape(b, d), self.nn1.weight, self.nn1.bias).view(b, 1, d)
        q = q.view(b, 1, h, d // h).transpose(1, 2)                                             # b, h, 1, dh
        kv = kv.view(b, n, 2, h, d // h).permute(2, 0, 3, 1, 4)                                 # 2, b, h, n, dh
        out = F.scaled_dot_product_attention(q, kv[0], kv[1], scale=self.scale).transpose(1, 2).reshape(b, 1, d)
        return self.nn1(out)


class _FeedForward(nn.Module):
    """MLP_Block (transformer.py:27-45)."""

    def __init__(self, dim, hidden, dropout):
        super().__init__()
        self.nn1 = nn.Linear(dim, hidden)
        nn.init.xavier_uniform_(self.nn1.weight)
        nn.init.normal_(self.nn1.bias, std=1e-6)
        self.af1 = nn.GELU()
        self.do1 = nn.Dropout(dropout)
        self.nn2 = nn.Linear(hidden, dim)
        nn.init.xavier_uniform_(self.nn2.weight)
        nn.init.normal_(self.nn2.bias, std=1e-6)
        self.do2 = nn.Dropout(dropout)

    def forward(self, x):
        return self.do2(self.forward_core(x))

    def forward_core(self, x, seed=None, salt=0):
        """forward(x) before its last dropout; with the training seed, GELU + dropout as _GeluDropout"""
        h = _train_linear(x, self.nn1.weight, self.nn1.bias)
        if (seed is not None and h.is_cuda and h.dtype == torch.float16 and h.numel() % 4 == 0 and
                getattr(self.af1, "approximate", None) == "none"):
            h = _GeluDropout.apply(h, _drop_p(self.do1), seed, salt)
        else:
            h = self.do1(self.af1(h))
        return _train_linear(h, self.nn2.weight, self.nn2.bias)


class _Encoder(nn.Module):
    def __init__(self, dim, depth, heads, mlp_dim, dropout):
        super().__init__()
        self.layers = nn.ModuleList([
            nn.ModuleList([_PreNorm(dim, _SelfAttention(dim, heads, dropout)),
                           _PreNorm(dim, _FeedForward(dim, mlp_dim, dropout))])
            for _ in range(depth)])

    fused_train = True      # training forward (GPU): _DropResLN residuals and _GeluDropout (with a seed)

    def _train_fused_ok(self, x):
        return (self.fused_train and hip_training(x) and x.dtype == torch.float32 and x.shape[-1] == 512 and
                all(pn.fn.norm.elementwise_affine for blk in self.layers for pn in blk))

    def _forward_train_fused(self, x, first_only, seed, start=None):
        """forward() of the training pass with every residual that feeds a LayerNorm as one _DropResLN
        (the residual add, its dropout and the next PreNorm's LayerNorm) and the MLP's GELU + dropout as
        _GeluDropout; the same operations and rounding points, the dropout masks from the kernels'
        hash (sites salted 2 li, 2 li + 1, 16 + li).  start: (z, x) -- the first PreNorm's output and its
        residual made already (_TokensLN); x is then unused."""
        L = len(self.layers)
        z, res = self.layers[0][0]._norm(x) if start is None else start
        for li, (att, ff) in enumerate(self.layers):
            a, f = att.fn.fn, ff.fn.fn
            if first_only and li == L - 1:
                y = a.forward_first_core(z)
                res = res[:, :1]
            else:
                y = a.forward_core(z)
            nrm = ff.fn.norm
            z, res = _DropResLN.apply(res, y, nrm.weight, nrm.bias, nrm.eps, _drop_p(a.do1), seed, 2 * li)
            y = f.forward_core(z, seed, 16 + li)
            if li + 1 < L:
                nrm = self.layers[li + 1][0].fn.norm
                z, res = _DropResLN.apply(res, y, nrm.weight, nrm.bias, nrm.eps, _drop_p(f.do2), seed, 2 * li + 1)
            else:
                return res + f.do2(y)

    def forward(self, x, first_only=False, seed=None):
        """first_only: return token 0 of the last block's output only ([b, 1, d]).  SCRIMPNet reads
        nothing else (net.py:140-141 takes x[:, 0]), so the last block's queries, output
        projection and MLP of tokens 1..16 are skipped; keys/values still see every token.
        seed: the training forward's device dropout seed (SCRIMPNet._train_seed): the fused training path."""
        if seed is not None and self._train_fused_ok(x):
            return self._forward_train_fused(x, first_only, seed)
        for li, (att, ff) in enumerate(self.layers):
            if first_only and li == len(self.layers) - 1:
                return ff(att.forward_first(x))
            x = ff(att(x))
        return x


class SCRIMPNet(nn.Module):
    def __init__(self, numChannel=None, num_agents=None, fov=None):
        super().__init__()
        W = NetParameters.NET_SIZE
        self.L = 16
        self.cT = W
        self.num_channel = NetParameters.NUM_CHANNEL if numChannel is None else numChannel
        self.num_agents = num_agents
        self.fov = fov
        self.conv1 = nn.Conv2d(self.num_channel, W // 4, 3, 1, 1)
        self.conv1a = nn.Conv2d(W // 4, W // 4, 3, 1, 1)
        self.conv1b = nn.Conv2d(W // 4, W // 4, 3, 1, 1)
        self.pool1 = nn.MaxPool2d(2)
        self.conv2 = nn.Conv2d(W // 4, W // 2, 2, 1, 1)
        self.conv2a = nn.Conv2d(W // 2, W // 2, 2, 1, 1)
        self.conv2b = nn.Conv2d(W // 2, W // 2, 2, 1, 1)
        self.pool2 = nn.MaxPool2d(2)
        self.conv3 = nn.Conv2d(W // 2, W - NetParameters.GOAL_REPR_SIZE, 3, 1, 0)
        self.fully_connected_1 = nn.Linear(NetParameters.VECTOR_LEN, NetParameters.GOAL_REPR_SIZE)
        self.fully_connected_2 = nn.Linear(W, W)
        self.fully_connected_3 = nn.Linear(W, W)
        self.token_wA = nn.Parameter(torch.empty(8, self.L, 512))
        nn.init.xavier_uniform_(self.token_wA)
        self.token_wV = nn.Parameter(torch.empty(8, 512, self.cT))
        nn.init.xavier_uniform_(self.token_wV)
        self.pos_embedding = nn.Parameter(torch.empty(1, self.L + 1, self.cT))
        nn.init.normal_(self.pos_embedding, std=0.02)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.cT))
        self.dropout = nn.Dropout(0.2)
        self.transformer = _Encoder(self.cT, 2, 16, 512, 0.2)
        self.nn_same = nn.Linear(self.cT, self.cT)
        nn.init.xavier_uniform_(self.nn_same.weight)
        nn.init.normal_(self.nn_same.bias, std=1e-6)
        self.policy_layer = nn.Linear(W, EnvParameters.N_ACTIONS)
        self.value_layer = nn.Linear(W, 1)
        self.cost_value_layer = nn.Linear(W, 1)
        self.blocking_layer = nn.Linear(W, 1)
        self.apply(_xavier_like)
        self.fused_acting = True      # no-grad GPU forward through acting.forward_fused (csrc/mapf_policy.hip)
        self.fused_attention = True   # short-sequence attention kernel (mapf_attention_f16) instead of SDPA
        self.fused_residual_ln = True  # residual + next LayerNorm in one pass (mapf_dropout_residual_layernorm)
        self.own_conv = True           # 128/256-channel convolutions as the MFMA implicit GEMM (mapf_conv_nhwc_f16)
        self.fused_linear = True       # 512x512 linears + their dropout/residual/LayerNorm or GELU epilogue, one launch
        self._h16 = {}                 # fp16 weights of the acting forward (acting.half)

    _OWN_CONV = _OWN_CONV          # the shapes of mapf_conv_nhwc_f16 (train_ops)
    # training forward on the GPU (grad, autocast) through the HIP ops of train_ops.py (train_ops.hip_training);
    # off: the plain torch-autocast forward the CPU runs (MIOpen, SDPA, nn.LayerNorm, torch dropout)
    hip_train = True
    fused_tokens = True            # training forward: tokens + dropout + first LayerNorm as _TokensLN
    _in_cast = False

    def _conv_nobias(self, x, m):
        """conv2d(x, m.weight) without the bias, fp16 NHWC: a plain GEMM where the kernel covers its whole
        unpadded input (conv3: 3x3 on 3x3 -> 1x1, as the acting path runs it; MIOpen's backward-data kernel
        took ~160 us for it in a 256 x 8-row update, profiles/r06h_update_profile_c3.txt), _HipConv for the
        MFMA kernel's shapes, else MIOpen"""
        w = m.weight
        co, ci, ks, _ = w.shape
        if (m.padding == (0, 0) and m.stride == (1, 1) and m.dilation == (1, 1) and m.groups == 1
                and x.shape[2] == ks and x.shape[3] == ks and x.dtype == torch.float16 and w.dtype == torch.float16
                and x.is_contiguous(memory_format=torch.channels_last)
                and w.is_contiguous(memory_format=torch.channels_last)):
            # [B, ks*ks*ci] x [co, ks*ks*ci]^T with K ordered (ky, kx, c): both operands are views of the
            # channels_last storage; autograd's GEMMs give the data and weight gradients
            B = x.shape[0]
            y = F.linear(x.permute(0, 2, 3, 1).reshape(B, -1), w.permute(0, 2, 3, 1).reshape(co, -1))
            return y.view(B, co, 1, 1)
        if self._own_conv_ok(x, m):
            return _HipConv.apply(x, w, m.padding[0], None, self._wt(m))
        return F.conv2d(x, w, None, m.stride, m.padding)

    def _wt(self, m):
        """m's flipped, transposed fp16 weight from this forward's _CastParams launch, or None"""
        return self.__dict__.get("_wt16", {}).get(m)

    def _own_conv_ok(self, x, m):
        """m's convolution of x runs on _HipConv (mapf_conv_nhwc_f16)"""
        w = m.weight
        co, ci, ks, _ = w.shape
        return ((ci, co, ks) in _OWN_CONV and w.dtype == torch.float16
                and x.dtype == torch.float16 and m.stride == (1, 1) and m.dilation == (1, 1) and m.groups == 1
                and m.padding[0] == m.padding[1] and m.padding[0] < ks
                and x.is_contiguous(memory_format=torch.channels_last)
                and w.is_contiguous(memory_format=torch.channels_last) and x.shape[0] > 0)

    def _conv_relu(self, x, m):
        """F.relu(m(x)) under autocast; on the GPU with grad, the convolution without its bias and
        _BiasReLU after it (NHWC fp16)"""
        if (hip_training(x) and m.bias is not None and m.out_channels % 4 == 0 and m.out_channels <= 1024 and
                m.weight.is_contiguous(memory_format=torch.channels_last)):
            if self._own_conv_ok(x, m):       # the bias + ReLU in the conv's epilogue
                b = m.bias if m.bias.dtype == torch.float16 else m.bias.to(torch.float16)
                return _HipConv.apply(x, m.weight, m.padding[0], b, self._wt(m))
            y = self._conv_nobias(x, m)
            if y.dtype == torch.float16 and y.is_contiguous(memory_format=torch.channels_last) and y.numel() > 0:
                b = m.bias if m.bias.dtype == torch.float16 else m.bias.to(torch.float16)
                return _BiasReLU.apply(y, b)
            return F.relu(y + m.bias.view(-1, 1, 1))
        return F.relu(m(x))

    def _conv_relu_pool(self, x, m, pool):
        """pool(F.relu(m(x))) under autocast; on the GPU with grad and a 2x2 / stride-2 max-pool, the
        convolution without its bias and _BiasReLUPool after it (NHWC fp16)"""
        ks = pool.kernel_size if isinstance(pool.kernel_size, int) else None
        st = pool.stride if isinstance(pool.stride, int) else None
        if (ks == 2 and st == 2 and pool.padding == 0 and pool.dilation == 1 and not pool.ceil_mode and
                hip_training(x) and m.bias is not None and m.out_channels % 4 == 0 and m.out_channels <= 1024 and
                m.weight.is_contiguous(memory_format=torch.channels_last)):
            r = self._conv_nobias(x, m)
            if (r.dtype == torch.float16 and r.is_contiguous(memory_format=torch.channels_last) and r.numel() > 0 and
                    r.shape[2] >= 2 and r.shape[3] >= 2):
                b = m.bias if m.bias.dtype == torch.float16 else m.bias.to(torch.float16)
                return _BiasReLUPool.apply(r, b)
            return pool(F.relu(r + m.bias.view(-1, 1, 1)))
        return pool(self._conv_relu(x, m))

    def _cast_names(self):
        """the parameters autocast would cast to fp16 in the training forward: every Conv2d / Linear
        weight and bias (LayerNorm's stay fp32; token_wA / token_wV are summed in fp32 first)"""
        names = getattr(self, "_cast_names_cache", None)
        if names is None:
            names = [f"{mn}.{pn}" for mn, m in self.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))
                     for pn, p in m.named_parameters(recurse=False)]
            self._cast_names_cache = names
        return names

    def _flip_names(self, names, own):
        """{conv module name: index in names of its weight} for the layers whose data gradient _HipConv runs
        on its own kernel (SCRIMPNet._OWN_CONV, channels_last weights): their flipped, transposed fp16 copies
        come from _CastParams' launch instead of a flip + copy per backward"""
        key = tuple(names)
        cache = self.__dict__.get("_flip_cache")
        if cache is None or cache[0] != key:
            out = {}
            for mn, m in self.named_modules():
                if isinstance(m, nn.Conv2d) and f"{mn}.weight" in names:
                    co, ci, ks, ks2 = m.weight.shape
                    if (ks == ks2 and (ci, co, ks) in _OWN_CONV and m.stride == (1, 1) and m.groups == 1
                            and m.dilation == (1, 1)):
                        out[mn] = names.index(f"{mn}.weight")
            cache = (key, out)
            self.__dict__["_flip_cache"] = cache
        out = cache[1]
        if not all(own[names[i]].is_contiguous(memory_format=torch.channels_last) for i in out.values()):
            return {}
        return out

    def _next_train_seed(self, x):
        """The training forward's dropout seed for the fused kernels (_DropResLN, _GeluDropout): an int64
        counter in device memory, incremented on the device by every training forward (so a captured
        update draws new masks on every replay; two models built from the same torch seed, or copies,
        draw the same).  None off the GPU training path."""
        if not hip_training(x):
            return None
        t = self.__dict__.get("_train_seed")
        if t is None or t.device != x.device:
            t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(x.device)
            self.__dict__["_train_seed"] = t
        t.add_(1)
        return t

    def weights_updated(self):
        """Forget the acting path's fp16 weight copies: an update replayed from a captured graph
        changes the parameters without bumping their version counters (acting.half's key)."""
        self._h16.clear()

    def forward(self, obs, vector, input_state=None):
        """Returns (policy, value, blocking, policy_sig, x, policy_logits, cost_value) like net.py:101-155.
        obs: [..., N, C, F, F] (any leading shape); the agent axis is num_agents (EnvParameters.N_AGENTS
        when not given at construction).  Acting on the GPU (no grad): acting.forward_fused.
        obs may be the packed observation (env.unpack_obs's input: int32 [..., N, WPA], one bit per
        cell; the net must know its fov): the fused acting forward reads it directly
        (mapf_conv_first_bits), every other path unpacks it into a scratch tensor first."""
        packed = obs.dtype == torch.int32
        if packed and not self.fov:
            raise ValueError("a packed observation needs the network's fov (SCRIMPNet(fov=...))")
        if self.fused_acting and obs.is_cuda and not torch.is_grad_enabled() and self.cT == 512:
            return acting.forward_fused(self, obs, vector)
        if packed:
            from .env import unpack_obs
            obs = unpack_obs(obs, self.num_channel, self.fov)
        if self.hip_train and obs.is_cuda and torch.is_grad_enabled() and not self._in_cast:
            # the same forward on fp16 copies of the conv / linear weights, made in one launch
            # (autocast would cast each weight on use and its ToCopyBackward each gradient)
            names = self._cast_names()
            own = dict(self.named_parameters())
            flips = self._flip_names(names, own)
            p16 = _CastParams.apply(tuple(flips.values()) if flips else (), *[own[n] for n in names])
            self._in_cast = True
            # the flipped weights of _HipConv's data gradients, by module (read in _conv_relu / _conv_nobias)
            self.__dict__["_wt16"] = {self.get_submodule(mn): wt for mn, wt in zip(flips, p16[len(names):])}
            try:
                return torch.func.functional_call(self, dict(zip(names, p16[:len(names)])), (obs, vector, input_state))
            finally:
                self._in_cast = False
                self.__dict__["_wt16"] = {}
        with torch.autocast(device_type=obs.device.type, enabled=obs.device.type == "cuda"):
            F_ = self.fov or obs.shape[-1]
            x = obs.reshape(-1, self.num_channel, F_, F_)
            if self.conv1.weight.is_contiguous(memory_format=torch.channels_last) and x.is_cuda:
                x = x.contiguous(memory_format=torch.channels_last)
            v = vector.reshape(-1, NetParameters.VECTOR_LEN)
            cr = self._conv_relu
            x = cr(x, self.conv1)
            x = cr(x, self.conv1a)
            x = self._conv_relu_pool(x, self.conv1b, self.pool1)
            x = cr(x, self.conv2)
            x = cr(x, self.conv2a)
            x = self._conv_relu_pool(x, self.conv2b, self.pool2)
            x = cr(x, self.conv3).flatten(1)
            g = F.relu(self.fully_connected_1(v))
            x3 = torch.cat((x, g), -1)
            fc2, fc3 = self.fully_connected_2, self.fully_connected_3
            h = _train_linear(F.relu(_train_linear(x3, fc2.weight, fc2.bias)), fc3.weight, fc3.bias)
            h = F.relu(h + x3).unsqueeze(1)                                   # [b, 1, 512]
            # tokeniser (net.py:124-130): sums over the 8 token matrices, softmax over a length-1 axis
            A = torch.matmul(h, self.token_wA.sum(0).transpose(0, 1))         # [b, 1, 16]
            A = A.transpose(1, 2).softmax(dim=-1)                             # [b, 16, 1]
            VV = torch.matmul(h, self.token_wV.sum(0))                        # [b, 1, 512]
            seed = self._next_train_seed(h)
            enc = self.transformer
            if (seed is not None and self.fused_tokens and enc._train_fused_ok(self.pos_embedding) and
                    A.dtype == torch.float32 and VV.dtype == torch.float16 and A.shape[1:] == (16, 1) and
                    VV.shape[1:] == (1, 512) and tuple(self.pos_embedding.shape) == (1, 17, 512) and
                    self.cls_token.numel() == 512 and self.cls_token.is_contiguous() and
                    self.pos_embedding.is_contiguous()):
                # tokens + dropout + the first PreNorm in one launch (_TokensLN)
                ln = enc.layers[0][0].fn.norm
                start = _TokensLN.apply(A.reshape(-1, 16).contiguous(), VV.reshape(-1, 512).contiguous(),
                                        self.cls_token, self.pos_embedding, ln.weight, ln.bias, ln.eps,
                                        _drop_p(self.dropout), seed, 32)
                x = enc._forward_train_fused(None, True, seed, start=start)
            else:
                T = A * VV                       # [b, 16, 512]: matmul(A, VV) over a length-1 axis
                x = torch.cat((self.cls_token.expand(T.shape[0], -1, -1), T), dim=1) + self.pos_embedding
                x = enc(self.dropout(x), first_only=True, seed=seed)
            ns = self.nn_same
            return self._heads(_train_linear(_train_linear(x[:, 0], ns.weight, ns.bias), ns.weight, ns.bias))

    def _heads(self, x):
        """the seven outputs (net.py:140-155) from the encoder's token 0 after nn_same, x: [b * agents, 512]"""
        x = x.reshape(-1, self.num_agents or EnvParameters.N_AGENTS, NetParameters.NET_SIZE)
        logits = self.policy_layer(x)
        policy = logits.softmax(dim=-1)
        policy_sig = torch.sigmoid(logits)
        value = self.value_layer(x)
        cost_value = self.cost_value_layer(x)
        blocking = torch.sigmoid(self.blocking_layer(x))
        return policy, value, blocking, policy_sig, x, logits, cost_value
