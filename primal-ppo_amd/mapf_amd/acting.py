"""SCRIMPNet's no-grad acting forward on the GPU, as plain functions of the net.

forward_fused(net, obs, vector) computes what net.forward computes under autocast, with the elementwise
epilogues, the short-sequence attention and the 128- / 256-channel convolutions in the HIP kernels of
csrc/mapf_policy.hip and csrc/mapf_conv.hip.  The fp16 weight copies are cached on the net (net._h16).
"""
import torch
import torch.nn.functional as F

from ._lib import call
from .config import NetParameters
from .train_ops import _OWN_CONV, _drop_p as drop

_HALF_VIEWS = {"sumT": lambda t: t.sum(0).transpose(0, 1), "sum": lambda t: t.sum(0),
               "ohwi": lambda t: t.permute(0, 2, 3, 1),        # conv weight for mapf_conv_nhwc_f16
               "ohwi2d": lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1),   # ... as a GEMM operand
               "k64": lambda t: F.pad(t.reshape(t.shape[0], -1), (0, 64 - t[0].numel())),   # mapf_conv_first_f32
               "q": lambda t: t[:t.shape[0] // 3], "kv": lambda t: t[t.shape[0] // 3:]}


def half(net, t, view=None):
    """fp16 copy of parameter t (or of a fixed view of it) for the acting forward, kept
    until t changes in place (optimizer step, load_state_dict bump its version) --
    autocast would re-cast every weight on every forward."""
    key = (id(t), view)
    ver = (t._version, t.data_ptr())
    hit = net._h16.get(key)
    if hit is None or hit[0] != ver:
        src = _HALF_VIEWS[view](t) if view else t
        hit = (ver, src.detach().to(torch.float16).contiguous())
        net._h16[key] = hit
    return hit[1]


def lin16(net, m, x):
    return F.linear(x, half(net, m.weight), None if m.bias is None else half(net, m.bias))


def forward_fused(net, obs, vector):
    """net.forward() for acting (no grad, GPU): the same operations at the same precision
    as forward() under autocast, with the elementwise epilogues in the HIP kernels of
    csrc/mapf_policy.hip -- conv bias + ReLU (+ max-pool) in one pass over each NHWC
    activation, LayerNorm written straight as the fp16 the next linear reads, dropout
    + residual add, GELU + dropout, tokeniser + positional embedding + dropout in one
    pass.  Dropout masks come from the kernels' counter-hash stream (seeded from torch's
    CPU generator), not from torch's.
    obs: float [..., C, F, F], or the packed observation int32 [..., WPA] (one bit per cell): conv1
    then reads the bits (mapf_conv_first_bits, bit-identical to conv1 on the unpacked floats)."""
    dev = obs.device
    packed = obs.dtype == torch.int32
    seeds = iter(torch.randint(0, 2 ** 62, (16,), dtype=torch.int64).tolist())
    h16 = lambda t, view=None: half(net, t, view)  # noqa: E731
    lin = lambda m, x: lin16(net, m, x)  # noqa: E731
    cl = torch.channels_last
    with torch.autocast(device_type="cuda"):
        F_ = net.fov or obs.shape[-1]
        if packed:
            x = obs.reshape(-1, obs.shape[-1]).contiguous()          # [agents, WPA]
            if not (net.own_conv and net.num_channel <= 7 and net.conv1.weight.shape[0] == 128):
                from .env import unpack_obs                           # no packed reader: a float scratch tensor
                x, packed = unpack_obs(x, net.num_channel, F_), False
        else:
            x = obs.reshape(-1, net.num_channel, F_, F_)
        v = vector.reshape(-1, NetParameters.VECTOR_LEN)

        def conv(x, m, pool=False):        # F.relu(conv(x)) (+ pool): bias and ReLU in the epilogue kernel
            b = h16(m.bias)
            co, ci, ks, _ = m.weight.shape
            if (pool and net.own_conv and (ci, co, ks) in ((128, 128, 3), (256, 256, 2)) and
                    x.is_contiguous(memory_format=cl)):
                # conv + bias + ReLU + 2x2 max-pool in one launch (mapf_conv_nhwc_pool_f16): the
                # conv's output never reaches HBM; a non-zero return code falls through to the two launches
                p = m.padding[0]
                B_, _, H_, W_ = x.shape
                Ho_, Wo_ = H_ + 2 * p - ks + 1, W_ + 2 * p - ks + 1
                yp = torch.empty((B_, co, Ho_ // 2, Wo_ // 2), dtype=torch.float16, device=dev, memory_format=cl)
                if call("mapf_conv_nhwc_pool_f16", x, h16(m.weight, "ohwi"), b, yp, B_, H_, W_, ci, co, ks, p,
                        check_rc=False) == 0:
                    return yp
            if net.own_conv and (ci, co, ks) in _OWN_CONV and x.is_contiguous(memory_format=cl):
                # the MFMA implicit GEMM (csrc/mapf_conv.hip); bias + ReLU in its epilogue unless pooled
                p = m.padding[0]
                B_, _, H_, W_ = x.shape
                y = torch.empty((B_, co, H_ + 2 * p - ks + 1, W_ + 2 * p - ks + 1), dtype=torch.float16,
                                device=dev, memory_format=cl)
                call("mapf_conv_nhwc_f16", x, h16(m.weight, "ohwi"), b, y, B_, H_, W_, ci, co, ks, p,
                     0 if pool else 1)
                if not pool:
                    return y
            elif (net.own_conv and m.padding[0] == 0 and x.shape[2] == ks and x.shape[3] == ks
                  and x.is_contiguous(memory_format=cl)):
                # a kernel covering its whole input (conv3: 3x3 on 3x3 -> 1x1) is a plain GEMM over
                # the NHWC pixel, K ordered (ky, kx, c): [B, KS*KS*Cin] x [Cout, KS*KS*Cin]^T
                B_ = x.shape[0]
                y = F.linear(x.permute(0, 2, 3, 1).reshape(B_, -1), h16(m.weight, "ohwi2d"))
                call("mapf_nhwc_bias_relu", y, b, B_, co)
                return y.view(B_, co, 1, 1)
            else:
                y = F.conv2d(x, h16(m.weight), None, m.stride, m.padding).contiguous(memory_format=cl)
            B_, C_, H_, W_ = y.shape
            if pool:     # a pooled layer's raw output takes bias + ReLU + pool in one pass
                out = torch.empty((B_, C_, H_ // 2, W_ // 2), dtype=y.dtype, device=dev, memory_format=cl)
                call("mapf_nhwc_bias_relu_pool2", y, b, out, B_, H_, W_, C_)
                return out
            call("mapf_nhwc_bias_relu", y, b, B_ * H_ * W_, C_)
            return y

        if packed:
            x1 = torch.empty((x.shape[0], 128, F_, F_), dtype=torch.float16, device=dev, memory_format=cl)
            call("mapf_conv_first_bits", x, h16(net.conv1.weight, "k64"), h16(net.conv1.bias), x1, x.shape[0],
                 net.num_channel, F_, F_, 128)
        elif (net.own_conv and net.num_channel <= 7 and net.conv1.weight.shape[0] == 128 and
                x.dtype == torch.float32 and x.is_contiguous()):
            # conv1 from the fp32 NCHW observation: cast, im2col, MFMA, bias + ReLU in one launch
            x1 = torch.empty((x.shape[0], 128, F_, F_), dtype=torch.float16, device=dev, memory_format=cl)
            call("mapf_conv_first_f32", x, h16(net.conv1.weight, "k64"), h16(net.conv1.bias), x1, x.shape[0],
                 net.num_channel, F_, F_, 128)
        else:
            x1 = conv(x.contiguous(memory_format=cl), net.conv1)
        x = conv(conv(x1, net.conv1a), net.conv1b, pool=True)
        x = conv(conv(conv(x, net.conv2), net.conv2a), net.conv2b, pool=True)
        x = conv(x, net.conv3).flatten(1)
        g = F.relu(lin(net.fully_connected_1, v))
        x3 = torch.cat((x, g), -1)
        h = lin(net.fully_connected_3, F.relu(lin(net.fully_connected_2, x3)))
        h = F.relu(h + x3).unsqueeze(1)                                   # [b, 1, 512]
        b = h.shape[0]
        hf = h.reshape(b, net.cT)                                         # 2-D GEMMs, not [b,1,512] bmm
        A = torch.matmul(hf, h16(net.token_wA, "sumT")).unsqueeze(-1).softmax(dim=-1)
        A = A.reshape(b, net.L).float().contiguous()                      # [b, 16] (all ones: length-1 softmax)
        VV = torch.matmul(hf, h16(net.token_wV, "sum")).contiguous()      # [b, 512] fp16
        xt = torch.empty(b, net.L + 1, net.cT, dtype=torch.float32, device=dev)
        cls, pos = net.cls_token.detach().contiguous(), net.pos_embedding.detach().contiguous()
        y0 = tok = None
        if net.fused_residual_ln:                      # tokens + the first LayerNorm in one pass
            layers = net.transformer.layers
            norm = layers[0][0].fn.norm
            y0 = torch.empty(xt.shape, dtype=torch.float16, device=dev)
            # the first block's fused out-projection recomputes the tokens (same mask bits): their
            # fp32 copy is then never written nor read back (mapf_linear512_tokens_residual_layernorm)
            recompute = (net.fused_linear and net.cT == 512 and len(layers) >= 2 and
                         layers[0][0].fn.fn.nn1.weight.shape == (512, 512))
            p_tok, seed_tok = drop(net.dropout), next(seeds)
            call("mapf_tokens_layernorm", None if recompute else xt, A, VV, cls, pos, b, net.L, net.cT, p_tok,
                 seed_tok, norm.weight, norm.bias, float(norm.eps), y0)
            if recompute:
                tok = (A, VV, cls, pos, p_tok, seed_tok)
        else:
            call("mapf_tokens", xt, A, VV, cls, pos, b, net.L, net.cT, drop(net.dropout), next(seeds))
        x = encoder_fused(net, xt, seeds, y0, tok)[:, 0]
        return net._heads(lin(net.nn_same, lin(net.nn_same, x)))


def encoder_fused(net, x, seeds, y0=None, tok=None):
    """net.transformer(x, first_only=True) on the fused epilogues; x fp32 [b, n, d] is
    updated in place (the residual stream) and token 0 after the last block returned; seeds: the
    iterator of the dropout sites' seeds; y0 is the first block's LayerNorm of x when the caller
    already computed it; tok = (A, VV, cls, pos, p, seed) when x was NOT written and the first fused
    out-projection recomputes it."""
    layers = net.transformer.layers
    b, n, d = x.shape
    h16 = lambda t, view=None: half(net, t, view)  # noqa: E731
    lin = lambda m, x: lin16(net, m, x)  # noqa: E731

    def ln(x, norm):                        # LayerNorm -> the fp16 the next linear reads
        y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        call("mapf_layernorm_f16", x, d, norm.weight, norm.bias, y, x.numel() // d, d, float(norm.eps))
        return y

    def residual(x, y, m, norm=None):       # x += dropout(y); then LayerNorm(x) -> fp16 if norm
        y = y.contiguous()
        if norm is None or not net.fused_residual_ln:
            call("mapf_dropout_residual", x, y, x.numel(), drop(m), next(seeds))
            return None if norm is None else ln(x, norm)
        z = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        call("mapf_dropout_residual_layernorm", x, y, norm.weight, norm.bias, z, x.numel() // d, d, float(norm.eps),
             drop(m), next(seeds))
        return z

    fused_lin = net.fused_linear and d == 512 and net.fused_residual_ln

    def lin_residual(m, inp, x, drop_m, norm, tok=None, x_every=1):   # x += dropout(m(inp)); LayerNorm(x)
        if not fused_lin or norm is None or m.weight.shape != (512, 512):
            assert tok is None
            return residual(x, lin(m, inp), drop_m, norm)
        inp = inp.contiguous()
        z = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        w, bias, eps = h16(m.weight), h16(m.bias), float(norm.eps)
        if tok is not None:                         # x = tokens (recomputed) + dropout(m(inp))
            A, VV, cls, pos, p_tok, seed_tok = tok
            call("mapf_linear512_tokens_residual_layernorm", inp, w, bias, x, norm.weight, norm.bias, z, x.shape[0],
                 x.shape[1] - 1, eps, drop(drop_m), next(seeds), A, VV, cls, pos, p_tok, seed_tok)
        elif x_every > 1:                           # only token 0's residual rows are read again
            call("mapf_linear512_residual_layernorm_rows", inp, w, bias, x, norm.weight, norm.bias, z,
                 x.numel() // d, eps, drop(drop_m), next(seeds), x_every)
        else:
            call("mapf_linear512_residual_layernorm", inp, w, bias, x, norm.weight, norm.bias, z, x.numel() // d,
                 eps, drop(drop_m), next(seeds))
        return z

    def lin_gelu(m, inp, drop_m):                   # dropout(gelu(m(inp))), one launch
        if not fused_lin or m.weight.shape != (512, 512):
            hid = lin(m, inp).contiguous()
            call("mapf_gelu_dropout_f16", hid, hid.numel(), drop(drop_m), next(seeds))
            return hid
        inp = inp.contiguous()
        hid = torch.empty(inp.shape[:-1] + (512,), dtype=torch.float16, device=inp.device)
        call("mapf_linear512_gelu_dropout", inp, h16(m.weight), h16(m.bias), hid, inp.numel() // 512, drop(drop_m),
             next(seeds))
        return hid

    def attend(q, k, v, rows, q_ts, kv_ts, a):     # fp16 [b, rows, d], heads concatenated
        o = torch.empty(b, rows, d, dtype=torch.float16, device=x.device)
        call("mapf_attention_f16", q, k, v, o, b, n, rows, q_ts, q_ts * (n if rows > 1 else 1), kv_ts, kv_ts * n,
             a.heads, d // a.heads, float(a.scale))
        return o

    y = ln(x, layers[0][0].fn.norm) if y0 is None else y0
    for li, (att, ff) in enumerate(layers):
        a = att.fn.fn
        hh = a.heads
        f = ff.fn.fn
        own_attn = net.fused_attention and hh * 32 == d == 512 and n <= 17
        if li < len(layers) - 1:
            qkv = lin(a.to_qkv, y)
            if own_attn:
                assert qkv.dtype == torch.float16 and qkv.is_contiguous()
                out = attend(qkv, qkv[..., d:], qkv[..., 2 * d:], n, 3 * d, 3 * d, a)
            else:
                qkv = qkv.view(b, n, 3, hh, d // hh).permute(2, 0, 3, 1, 4)
                out = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], scale=a.scale)
                out = out.transpose(1, 2).reshape(b, n, d)
            yf = lin_residual(a.nn1, out, x, a.do1, ff.fn.norm, tok if li == 0 else None)
        else:                               # the last block: token 0's query only (see _Encoder)
            w, bias = a.to_qkv.weight, a.to_qkv.bias
            q = F.linear(y[:, 0], h16(w, "q"), h16(bias, "q"))
            kv = F.linear(y, h16(w, "kv"), h16(bias, "kv"))
            if own_attn:
                assert q.dtype == kv.dtype == torch.float16 and q.is_contiguous() and kv.is_contiguous()
                out = attend(q, kv, kv[..., d:], 1, d, 2 * d, a)
            else:
                q = q.view(b, 1, hh, d // hh).transpose(1, 2)
                kv = kv.view(b, n, 2, hh, d // hh).permute(2, 0, 3, 1, 4)
                out = F.scaled_dot_product_attention(q, kv[0], kv[1], scale=a.scale)
                out = out.transpose(1, 2).reshape(b, 1, d)
            x = x[:, :1].contiguous()
            yf = lin_residual(a.nn1, out, x, a.do1, ff.fn.norm)
        hid = lin_gelu(f.nn1, yf, f.do1)
        # before the last block only token 0 of the stream is carried on (x[:, :1] below)
        y = lin_residual(f.nn2, hid, x, f.do2, layers[li + 1][0].fn.norm if li + 1 < len(layers) else None,
                         x_every=n if li + 2 == len(layers) and x.shape[1] == n else 1)
    return x
