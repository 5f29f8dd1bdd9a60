"""The HIP training kernels of csrc/mapf_policy.hip as torch.autograd.Functions, and `_train_linear`.

net.py's training forward (GPU, grad enabled, under autocast: `hip_training`) dispatches to these in
place of torch's ops; each class documents the torch chain it stands for.  Every launch goes through
`_lib.call`.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib

# (Cin, Cout, kernel) of mapf_conv_nhwc_f16; (256, 128, 2) is conv2's data gradient (_HipConv)
_OWN_CONV = {(128, 128, 3), (128, 256, 2), (256, 256, 2), (256, 128, 2)}


def hip_training(x):
    """x is on the HIP training path: SCRIMPNet.hip_train, on the GPU, grad enabled, under autocast.
    Off (or on the CPU) the forward is plain torch under autocast: MIOpen, SDPA, nn.LayerNorm, torch dropout."""
    from .net import SCRIMPNet                  # net.py imports this module
    return SCRIMPNet.hip_train and x.is_cuda and torch.is_grad_enabled() and torch.is_autocast_enabled("cuda")


def _drop_p(m):
    """a Dropout module's probability as the forward applies it (0 in eval mode)"""
    return float(m.p) if m.training else 0.0


def _layernorm_bwd(x, x_stride, weight, dz, dres, eps, rows, work_floats=2 * 512 * 512, drop=None):
    """LayerNorm's backward over `rows` 512-wide fp32 rows of x with the residual's gradient dres added to dx
    (mapf_layernorm_bwd_f16); with drop = (p, seed, salt) also the dropped fp16 branch's gradient dy
    (mapf_layernorm_dropout_bwd_f16, contiguous x).  A missing dz is zeros, a missing dres NULL.
    Returns (dx fp32 [rows, 512], dy or None, dgamma, dbeta, work)."""
    dev = x.device
    if dz is None:
        dz = torch.zeros(rows, 512, dtype=torch.float16, device=dev)
    dz = dz.reshape(rows, 512).to(torch.float16).contiguous()
    if dres is not None:
        dres = dres.reshape(rows, 512).to(torch.float32).contiguous()
    dx = torch.empty(rows, 512, dtype=torch.float32, device=dev)
    dy = None if drop is None else torch.empty(rows, 512, dtype=torch.float16, device=dev)
    dg = torch.empty(512, dtype=torch.float32, device=dev)
    db = torch.empty(512, dtype=torch.float32, device=dev)
    work = torch.empty(work_floats, dtype=torch.float32, device=dev)
    if drop is None:
        _lib.call("mapf_layernorm_bwd_f16", x, x_stride, weight, dz, dres, dx, dg, db, work, rows, 512, eps)
    else:
        p, seed, salt = drop
        _lib.call("mapf_layernorm_dropout_bwd_f16", x, weight, dz, dres, dx, dy, dg, db, work, rows, 512, eps, p,
                  seed, salt)
    return dx, dy, dg, db, work


def _relu_bias_bwd(y, dy):
    """(dx, dbias) of y = relu(x + b) on NHWC fp16 (mapf_relu_bias_bwd_f16): the ReLU mask and the bias
    gradient (fp32 sums rounded to fp16, as torch's fp16 sum) in one pass"""
    C = y.shape[1]
    dx = torch.empty_like(y)
    db = torch.empty(C, dtype=torch.float16, device=y.device)
    work = torch.empty(512 * C, dtype=torch.float32, device=y.device)
    _lib.call("mapf_relu_bias_bwd_f16", y, dy, dx, db, work, y.numel() // C, C)
    return dx, db


class _HipLayerNorm(torch.autograd.Function):
    """fp16(LayerNorm(x)) of the TRAINING forward under autocast -- what the next fp16 linear reads
    (autocast runs layer_norm in fp32 and casts at the linear): the forward is mapf_layernorm_f16
    (the acting path's kernel), the backward mapf_layernorm_bwd_f16 (dx in fp32, dgamma / dbeta
    summed over the rows).  Replaces torch's LayerNorm forward, its two backward kernels and the
    fp32 <-> fp16 casts on either side (tools/profile_update.py).  x: fp32 [.., 512]."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        """returns (z, x viewed): the PreNorm adds the second output back as its residual, so the
        residual path's gradient arrives in backward and is added to dx by the kernel"""
        ctx.set_materialize_grads(False)
        x2 = x.reshape(-1, 512)
        if x2.stride(0) % 4 or x2.stride(1) != 1:
            x2 = x2.contiguous()
        rows = x2.shape[0]
        z = torch.empty(rows, 512, dtype=torch.float16, device=x.device)
        _lib.call("mapf_layernorm_f16", x2, x2.stride(0), weight, bias, z, rows, 512, float(eps))
        ctx.save_for_backward(x2, weight)
        ctx.eps, ctx.shape = float(eps), x.shape
        return z.view(*x.shape[:-1], 512), x.view_as(x)

    @staticmethod
    def backward(ctx, dz, dres):
        x2, weight = ctx.saved_tensors
        dx, _, dg, db, _ = _layernorm_bwd(x2, x2.stride(0), weight, dz, dres, ctx.eps, x2.shape[0])
        return dx.view(ctx.shape), dg, db, None


def _cast_multi(name, srcs, dsts, *extra):
    """one multi-tensor cast launch: pointer arrays of srcs / dsts, their element counts, `extra` arrays"""
    k = len(srcs)
    arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])  # noqa: E731
    _lib.call(name, arr(srcs), arr(dsts), (ctypes.c_int64 * k)(*[t.numel() for t in srcs]), *extra, k,
              device=srcs[0].device)


class _CastParams(torch.autograd.Function):
    """fp16 copies of fp32 parameters in ONE launch (mapf_cast_f32_to_f16_multi), their gradients back
    to fp32 in one (mapf_cast_f16_to_f32_multi): what autocast's per-weight casts and their
    ToCopyBackward nodes compute (round to nearest even; exact), in 2 launches instead of ~90 per
    update (tools/profile_update.py)."""

    @staticmethod
    def dense(t):
        """storage is exactly the tensor's numel elements (any dense layout: contiguous, channels_last)"""
        return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))

    @staticmethod
    def forward(ctx, flips, *params):
        """flips: indices of channels_last conv weights whose flipped, transposed fp16 copy ([Cin][Cout][ks][ks],
        channels_last: _HipConv's data-gradient weight) is returned too, after the plain copies, from the
        same launch (mapf_cast_f32_to_f16_multi_flip); those copies carry no gradient"""
        ctx.set_materialize_grads(False)
        assert all(_CastParams.dense(p) for p in params)
        ctx.layouts = [(p.shape, p.stride()) for p in params]
        outs = [torch.empty_strided(p.shape, p.stride(), dtype=torch.float16, device=p.device) for p in params]
        if not flips:
            _cast_multi("mapf_cast_f32_to_f16_multi", params, outs)
            return tuple(outs)
        fl = [params[i] for i in flips]
        assert all(w.dim() == 4 and w.shape[2] == w.shape[3] and w.is_contiguous(memory_format=torch.channels_last)
                   for w in fl)
        wts = [torch.empty((w.shape[1], w.shape[0], w.shape[2], w.shape[3]), dtype=torch.float16, device=w.device,
                           memory_format=torch.channels_last) for w in fl]
        k = len(params) + len(fl)
        co = (ctypes.c_int32 * k)(*([0] * len(params) + [w.shape[0] for w in fl]))
        kk = (ctypes.c_int32 * k)(*([0] * len(params) + [w.shape[2] for w in fl]))
        _cast_multi("mapf_cast_f32_to_f16_multi_flip", list(params) + fl, outs + wts, co, kk)
        ctx.mark_non_differentiable(*wts)
        return tuple(outs + wts)

    @staticmethod
    def backward(ctx, *grads):
        grads = grads[:len(ctx.layouts)]                 # the flipped copies carry none
        live = [i for i, g in enumerate(grads) if g is not None]
        outs = [None] * len(grads)
        if live:
            src, dst = [], []
            for i in live:
                shape, stride = ctx.layouts[i]
                g = grads[i]
                if g.stride() != stride:        # the parameter's own layout (AccumulateGrad keeps it)
                    g = torch.empty_strided(shape, stride, dtype=g.dtype, device=g.device).copy_(g)
                src.append(g)
                dst.append(torch.empty_strided(shape, stride, dtype=torch.float32, device=g.device))
            _cast_multi("mapf_cast_f16_to_f32_multi", src, dst)
            for i, d in zip(live, dst):
                outs[i] = d
        return (None,) + tuple(outs)


class _BiasReLU(torch.autograd.Function):
    """relu(y + b) in place on a convolution's NHWC fp16 output (mapf_nhwc_bias_relu, the acting
    path's epilogue), for the TRAINING forward's conv layers run without MIOpen's bias; backward
    _relu_bias_bwd -- in place of MIOpen's bias add, torch's ReLU and threshold backward and its
    bias-gradient reduction.  y: fp16 channels_last, b: fp16 [C]."""

    @staticmethod
    def forward(ctx, y, b):
        C = y.shape[1]
        _lib.call("mapf_nhwc_bias_relu", y, b, y.numel() // C, C)
        ctx.mark_dirty(y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        return _relu_bias_bwd(y, dy.contiguous(memory_format=torch.channels_last))


class _BiasReLUPool(torch.autograd.Function):
    """maxpool2x2(relu(r + b)) from a convolution's raw NHWC fp16 output r in one pass
    (mapf_nhwc_bias_relu_pool2, the acting path's epilogue) for the TRAINING forward's pooled layers
    (conv1b, conv2b; net.py:106-111); backward mapf_relu_bias_pool_bwd_f16: torch's max_pool2d argmax
    routing, the ReLU mask and the bias gradient in one pass -- in place of the bias + ReLU pass, torch's
    max-pool forward / backward and the masked-gradient pass."""

    @staticmethod
    def forward(ctx, r, b):
        B, C, H, W = r.shape
        p = torch.empty((B, C, H // 2, W // 2), dtype=torch.float16, device=r.device,
                        memory_format=torch.channels_last)
        _lib.call("mapf_nhwc_bias_relu_pool2", r, b, p, B, H, W, C)
        ctx.save_for_backward(r, b)
        return p

    @staticmethod
    def backward(ctx, dp):
        r, b = ctx.saved_tensors
        B, C, H, W = r.shape
        dp = dp.contiguous(memory_format=torch.channels_last)
        dr = torch.empty_like(r)
        db = torch.empty(C, dtype=torch.float16, device=r.device)
        work = torch.empty(512 * C, dtype=torch.float32, device=r.device)
        _lib.call("mapf_relu_bias_pool_bwd_f16", r, b, dp, dr, db, work, B, H, W, C)
        return dr, db


class _HipConv(torch.autograd.Function):
    """conv2d(x, w) without bias (stride 1, fp16 NHWC, net.py:104-112) for the TRAINING forward's
    128- / 256-channel layers on the acting path's MFMA implicit GEMM (mapf_conv_nhwc_f16, raw fp16
    output: fp32 accumulation, one rounding, as MIOpen's); the bias + ReLU (+ pool) follow in _BiasReLU /
    _BiasReLUPool.  Backward: the data gradient is the same kernel run over dy with the flipped,
    transposed weight (dx = conv(dy, w[:, :, ::-1, ::-1]^T), padding ks - 1 - pad) wherever that
    shape is one the kernel has (_OWN_CONV: every layer from conv1a to conv2b), else MIOpen's;
    the weight gradient is MIOpen's (aten.convolution_backward).  In place of MIOpen's forward and data
    gradient (0.28 + 0.48 ms of a 256 x 8-row update, profiles/r06_update_profile_c3.txt)."""

    @staticmethod
    def forward(ctx, x, w, pad, b=None, wt=None):
        B, Cin, H, W = x.shape
        Cout, _, ks, _ = w.shape
        y = torch.empty((B, Cout, H + 2 * pad - ks + 1, W + 2 * pad - ks + 1), dtype=torch.float16, device=x.device,
                        memory_format=torch.channels_last)
        # a channels_last [Cout][Cin][ks][ks] weight is [Cout][ks][ks][Cin] in memory: the kernel's packed form;
        # with b: relu(fp16(fp16(acc) + b)) in the epilogue, what _BiasReLU's pass writes
        _lib.call("mapf_conv_nhwc_f16", x, w, b, y, B, H, W, Cin, Cout, ks, pad, 0 if b is None else 1)
        ctx.save_for_backward(x, w, None if b is None else y, wt)
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, wt = ctx.saved_tensors
        pad = ctx.pad
        B, Cin, H, W = x.shape
        Cout, _, ks, _ = w.shape
        dy = dy.contiguous(memory_format=torch.channels_last)
        db = None
        if y is not None:                       # the fused bias + ReLU: _BiasReLU's backward first
            dy, db = _relu_bias_bwd(y, dy)
        own_dx = ctx.needs_input_grad[0] and (Cout, Cin, ks) in _OWN_CONV
        mask = [ctx.needs_input_grad[0] and not own_dx, ctx.needs_input_grad[1], False]
        dx = dw = None
        if any(mask):
            gx, gw, _ = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1,
                                                            mask)
            dx = gx if mask[0] else None
            dw = gw if mask[1] else None
        if own_dx:
            if wt is None:                      # else _CastParams made it (SCRIMPNet._flip_names)
                wt = w.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)  # [Cin][ks][ks][Cout]
            dx = torch.empty(x.shape, dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
            _lib.call("mapf_conv_nhwc_f16", dy, wt, None, dx, B, dy.shape[2], dy.shape[3], Cout, Cin, ks,
                      ks - 1 - pad, 0)
        return dx, dw, None, db, None


class _TokensLN(torch.autograd.Function):
    """The TRAINING forward's tokeniser tail and the first PreNorm in one pass (round 6):
    x = dropout(cat(cls, A * VV) + pos) fp32, z = fp16(LayerNorm(x)) -- mapf_tokens_layernorm_train, the
    ops and roundings of SCRIMPNet.forward's torch chain (net.py:124-130, transformer.py:7-24; the mask is
    the kernels' counter hash from the device seed, salt 32).  Backward: LayerNorm's with the residual's
    gradient (mapf_layernorm_bwd_f16), then mapf_tokens_train_bwd: the dropout mask, dA, dVV (fp16) and the
    sums over the batch for pos and cls.  In place of torch's mul, cat, add, dropout, LayerNorm launches and
    their backward's mul / sum / masked-scale passes (~0.29 ms of a 256 x 8-row update,
    profiles/r06n_update_shapes.txt).  A: fp32 [B, 16]; VV: fp16 [B, 512]; returns (z [B, 17, 512] fp16,
    x [B, 17, 512] fp32: the first block's residual)."""

    @staticmethod
    def forward(ctx, A, VV, cls, pos, weight, bias, eps, p, seed, salt):
        ctx.set_materialize_grads(False)
        B = A.shape[0]
        x = torch.empty(B, 17, 512, dtype=torch.float32, device=A.device)
        z = torch.empty(B, 17, 512, dtype=torch.float16, device=A.device)
        _lib.call("mapf_tokens_layernorm_train", x, A, VV, cls, pos, B, 16, float(p), seed, int(salt), weight, bias,
                  float(eps), z)
        ctx.save_for_backward(x, A, VV, weight, seed)
        ctx.eps, ctx.p, ctx.salt, ctx.shapes = float(eps), float(p), int(salt), (cls.shape, pos.shape)
        return z, x

    @staticmethod
    def backward(ctx, dz, dres):
        x, A, VV, weight, seed = ctx.saved_tensors
        B = A.shape[0]
        dev = x.device
        # the work space is mapf_tokens_train_bwd's partials (larger than LayerNorm's own)
        dx, _, dg, db, work = _layernorm_bwd(x, 512, weight, dz, dres, ctx.eps, B * 17, work_floats=512 * 17 * 512)
        dA = torch.empty(B, 16, dtype=torch.float32, device=dev)
        dVV = torch.empty(B, 512, dtype=torch.float16, device=dev)
        dpos = torch.empty(17, 512, dtype=torch.float32, device=dev)
        dcls = torch.empty(512, dtype=torch.float32, device=dev)
        _lib.call("mapf_tokens_train_bwd", dx, A, VV, dA, dVV, dpos, dcls, work, B, 16, ctx.p, seed, ctx.salt)
        cs, ps = ctx.shapes
        return dA, dVV, dcls.view(cs), dpos.view(ps), dg, db, None, None, None, None


class _DropResLN(torch.autograd.Function):
    """The TRAINING forward's residual + next PreNorm in one pass (round 6): x_out = res + dropout(y),
    z = fp16(LayerNorm(x_out)) -- mapf_dropout_residual_layernorm_train; backward
    mapf_layernorm_dropout_bwd_f16: LayerNorm's backward with the residual gradient (as _HipLayerNorm),
    the dropped branch's fp16 gradient and dgamma / dbeta in one pass.  In place of torch's dropout
    forward / backward, the fp32 add and a separate LayerNorm launch at every residual that feeds a
    LayerNorm (transformer.py:7-24, 64-85).  The dropout mask is the kernels' counter hash seeded from
    `seed` (SCRIMPNet._train_seed, int64 [1] in device memory, incremented by every training forward --
    also inside a captured update) and the site's salt.  res: fp32 [.., 512] (a strided view allowed),
    y: fp16 [.., 512]."""

    @staticmethod
    def forward(ctx, res, y, weight, bias, eps, p, seed, salt):
        ctx.set_materialize_grads(False)
        rows = res.numel() // 512
        r2 = res.reshape(rows, 512)
        if r2.stride(1) != 1 or r2.stride(0) % 4:
            r2 = r2.contiguous()
        y2 = y.reshape(rows, 512).contiguous()
        xo = torch.empty(rows, 512, dtype=torch.float32, device=res.device)
        z = torch.empty(rows, 512, dtype=torch.float16, device=res.device)
        _lib.call("mapf_dropout_residual_layernorm_train", r2, r2.stride(0), y2, xo, weight, bias, z, rows, 512,
                  float(eps), float(p), seed, int(salt))
        ctx.save_for_backward(xo, weight, seed)
        ctx.meta = (float(eps), float(p), int(salt), res.shape, y.shape)
        out_shape = tuple(res.shape[:-1]) + (512,)
        return z.view(out_shape), xo.view(out_shape)

    @staticmethod
    def backward(ctx, dz, dxo):
        xo, weight, seed = ctx.saved_tensors
        eps, p, salt, res_shape, y_shape = ctx.meta
        dx, dy, dg, db, _ = _layernorm_bwd(xo, 512, weight, dz, dxo, eps, xo.shape[0], drop=(p, seed, salt))
        return dx.view(res_shape), dy.view(y_shape), dg, db, None, None, None, None


class _GeluDropout(torch.autograd.Function):
    """dropout(gelu(h)) of the TRAINING forward's MLP (transformer.py:27-45, af1 + do1) in one pass each
    way (round 6): mapf_gelu_dropout_train_f16 / mapf_gelu_dropout_bwd_f16 -- torch's fp16 GELU, dropout,
    masked_scale and GeluBackward kernels in two launches; the mask as _DropResLN's.  h: fp16."""

    @staticmethod
    def forward(ctx, h, p, seed, salt):
        h = h.contiguous()
        out = torch.empty_like(h)
        _lib.call("mapf_gelu_dropout_train_f16", h, out, h.numel(), float(p), seed, int(salt))
        ctx.save_for_backward(h, seed)
        ctx.meta = (float(p), int(salt))
        return out

    @staticmethod
    def backward(ctx, dout):
        h, seed = ctx.saved_tensors
        p, salt = ctx.meta
        dout = dout.to(torch.float16).contiguous()
        dh = torch.empty_like(h)
        _lib.call("mapf_gelu_dropout_bwd_f16", h, dout, dh, h.numel(), p, seed, salt)
        return dh, None, None, None


class _HipAttention(torch.autograd.Function):
    """softmax(q k^T * scale) v over <= 32 tokens, 16 heads of 32, for the TRAINING forward:
    mapf_attention_f16 forward, mapf_attention_bwd_f16 backward (csrc/mapf_policy.hip) in place of
    SDPA's flash kernels, which are tiled for long sequences.  q: `rows` tokens at column q_off of
    qsrc [b, t, wq] (or [b, wq]); k, v at columns k_off, v_off of kvsrc [b, n, wkv]; both fp16
    and contiguous -- qsrc may be kvsrc (the fused qkv projection), then one gradient comes back.
    Returns [b, rows, 512] fp16."""

    @staticmethod
    def _meta(qsrc, kvsrc):
        b, n, wkv = kvsrc.shape
        wq = qsrc.shape[-1]
        q_ss = wq * (qsrc.shape[1] if qsrc.dim() == 3 else 1)
        return b, n, wq, q_ss, wkv, n * wkv

    @staticmethod
    def forward(ctx, qsrc, kvsrc, rows, q_off, k_off, v_off, scale):
        b, n, wq, q_ss, kv_ts, kv_ss = _HipAttention._meta(qsrc, kvsrc)
        out = torch.empty(b, rows, 512, dtype=torch.float16, device=qsrc.device)
        e = 2                                                      # bytes per fp16 element
        _lib.call("mapf_attention_f16", qsrc.data_ptr() + e * q_off, kvsrc.data_ptr() + e * k_off,
                  kvsrc.data_ptr() + e * v_off, out, b, n, rows, wq, q_ss, kv_ts, kv_ss, 16, 32, float(scale))
        ctx.save_for_backward(qsrc, kvsrc, out)
        ctx.args = (rows, q_off, k_off, v_off, scale, qsrc.data_ptr() == kvsrc.data_ptr())
        return out

    @staticmethod
    def backward(ctx, dout):
        qsrc, kvsrc, out = ctx.saved_tensors
        rows, q_off, k_off, v_off, scale, same = ctx.args
        b, n, wq, q_ss, kv_ts, kv_ss = _HipAttention._meta(qsrc, kvsrc)
        dout = dout.contiguous()
        gq = torch.empty_like(qsrc)
        gkv = gq if same else torch.empty_like(kvsrc)
        p = lambda t, off: t.data_ptr() + 2 * off  # noqa: E731  (fp16 columns)
        _lib.call("mapf_attention_bwd_f16", p(qsrc, q_off), p(kvsrc, k_off), p(kvsrc, v_off), out, dout,
                  p(gq, q_off), p(gkv, k_off), p(gkv, v_off), b, n, rows, wq, q_ss, kv_ts, kv_ss, 512, rows * 512, 16,
                  32, float(scale))
        return gq, (None if same else gkv), None, None, None, None, None


class _SplitKLinear(torch.autograd.Function):
    """F.linear under fp16 autocast for the TRAINING forward's 17-token layers (34,816 rows at 2,048
    agents): the forward is autocast's (fp16 operands, one GEMM with the bias), the input gradient
    one GEMM; the WEIGHT gradient is split over SPLIT row chunks, one batched GEMM with fp32 partial
    products summed in fp32, then rounded to fp16 as autograd's one-GEMM fp16 weight gradient is
    (so an fp16 overflow still reaches GradScaler's found-inf).  hipBLASLt's one GEMM has only
    (out / 64) x (in / 128) output tiles for the 34,816-deep reduction -- 32 tiles on 256 CUs for a
    512 x 512 weight (tools/profile_update.py)."""

    SPLIT = 16                      # 8 -> 16: -0.06 / -0.11 ms per 256 x 8 / 256 x 16 update (profiles/r06ze_ab_split*)
    MIN_ROWS = 8192                 # _train_linear takes this form from this many rows on
    out_dtype_ok = None             # torch.bmm(..., out_dtype=float32) on this build (decided once, _fp32_bmm)

    @staticmethod
    def _fp32_bmm(a, c):
        """torch.bmm(a, c, out_dtype=float32), or None when this torch build has no such overload --
        decided once, by the call's signature error (TypeError / NotImplementedError) only: any other
        error (an OOM, a launch failure) propagates instead of switching every later gradient to fp16
        partial products"""
        if _SplitKLinear.out_dtype_ok is False:
            return None
        try:
            parts = torch.bmm(a, c, out_dtype=torch.float32)
        except (TypeError, NotImplementedError) as e:
            import warnings
            warnings.warn(f"torch.bmm(..., out_dtype=float32) unavailable ({e}): split weight gradients use fp16 "
                          f"partial products", RuntimeWarning)
            _SplitKLinear.out_dtype_ok = False
            return None
        _SplitKLinear.out_dtype_ok = True
        return parts

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float16)
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.bias_dtype = b.dtype if b is not None else None
        return F.linear(x, w, b)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        n_out, n_in = w.shape
        gy2 = gy.reshape(-1, n_out)
        x2 = x.reshape(-1, n_in)
        gx = (gy2 @ w).view(x.shape) if ctx.needs_input_grad[0] else None
        S = _SplitKLinear.SPLIT
        r = gy2.shape[0] // S
        a = gy2.view(S, r, n_out).transpose(1, 2)
        c = x2.view(S, r, n_in)
        parts = _SplitKLinear._fp32_bmm(a, c)
        if parts is None:
            parts = torch.bmm(a, c).float()
        gw = parts.sum(0).to(torch.float16).to(w.dtype)
        gb = None
        if ctx.needs_input_grad[2] and n_out % 4:
            gb = gy2.sum(0).to(ctx.bias_dtype)
        elif ctx.needs_input_grad[2]:   # bias gradient: the column sums of gy
            gy2 = gy2.contiguous()
            gb = torch.empty(n_out, dtype=torch.float16, device=gy.device)
            work = torch.empty(512 * n_out, dtype=torch.float32, device=gy.device)
            _lib.call("mapf_colsum_f16", gy2, gb, work, gy2.shape[0], n_out)
            gb = gb.to(ctx.bias_dtype)
        return gx, gw, gb


class _QKVFirst(torch.autograd.Function):
    """The last encoder block's projections (forward_first_core) from ONE to_qkv weight [3d, d]: token 0's
    query q = x[:, 0] W_q^T + b_q and every token's keys / values kv = x W_kv^T + b_kv, with one backward:
    the input gradient is kv's GEMM with token 0's query gradient accumulated into its rows (addmm_), so no
    zero-filled [b, n, d] select gradient and no add; the weight and bias gradients are written into one
    [3d, d] / [3d] tensor, so no zero-filled slice gradients and adds either.  kv's weight gradient is
    _SplitKLinear's (split-K, fp32 partials, rounded to fp16), q's one GEMM; the bias gradients
    mapf_colsum_f16.  x: fp16 [b, n, d] contiguous; w, b fp16 (the training forward's _CastParams copies)."""

    @staticmethod
    def forward(ctx, x, w, b):
        d = x.shape[-1]
        ctx.save_for_backward(x, w)
        return torch.addmm(b[:d], x[:, 0], w[:d].t()), F.linear(x, w[d:], b[d:])

    @staticmethod
    def backward(ctx, dq, dkv):
        x, w = ctx.saved_tensors
        B, n, d = x.shape
        dev = x.device
        x2 = x.reshape(-1, d)
        dq = torch.zeros(B, d, dtype=x.dtype, device=dev) if dq is None else dq.contiguous()
        dkv2 = (torch.zeros(B * n, 2 * d, dtype=x.dtype, device=dev) if dkv is None else dkv.reshape(-1, 2 * d)
                .contiguous())
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = (dkv2 @ w[d:]).view(B, n, d)
            gx[:, 0].addmm_(dq, w[:d])
        if ctx.needs_input_grad[1]:
            gw = torch.empty(3 * d, d, dtype=torch.float16, device=dev)
            torch.mm(dq.t(), x[:, 0], out=gw[:d])
            S = _SplitKLinear.SPLIT
            R = dkv2.shape[0]
            parts = None
            if R % S == 0:
                a, c = dkv2.view(S, R // S, 2 * d).transpose(1, 2), x2.view(S, R // S, d)
                parts = _SplitKLinear._fp32_bmm(a, c)
                if parts is None:
                    parts = torch.bmm(a, c).float()
            if parts is not None:
                gw[d:].copy_(parts.sum(0))
            else:
                torch.mm(dkv2.t(), x2, out=gw[d:])
            gw = gw.to(w.dtype)
        if ctx.needs_input_grad[2]:
            gb = torch.empty(3 * d, dtype=torch.float16, device=dev)
            work = torch.empty(512 * 2 * d, dtype=torch.float32, device=dev)    # one work space for both sums
            for g2, lo, C in ((dq, 0, d), (dkv2, d, 2 * d)):
                _lib.call("mapf_colsum_f16", g2, gb.data_ptr() + 2 * lo, work, g2.shape[0], C)
        return gx, gw, gb


class _LinearBG(torch.autograd.Function):
    """F.linear(x, w, b) on fp16 operands for the training forward's short linears (token 0's and the
    fully connected layers: 2-D, rows < _SplitKLinear.MIN_ROWS): the same addmm forward and the same
    two GEMMs backward as torch's AddmmBackward, the bias gradient from mapf_colsum_f16's one-launch
    column sum (fp32, fixed order, rounded to fp16) in place of torch's fp16 reduction (~15 us per layer,
    8 layers per update: profiles/r06n_update_shapes.txt).  x: fp16 [rows, in] (strided rows allowed)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy.mm(w) if ctx.needs_input_grad[0] else None
        gw = x.t().mm(gy).t() if ctx.needs_input_grad[1] else None
        gb = None
        if ctx.needs_input_grad[2]:
            n_out = gy.shape[1]
            gb = torch.empty(n_out, dtype=torch.float16, device=gy.device)
            # the partials path's size whatever the rows: mapf_colsum_f16 also takes that path for a
            # gradient that is not 16-byte aligned
            work = torch.empty(512 * n_out, dtype=torch.float32, device=gy.device)
            _lib.call("mapf_colsum_f16", gy, gb, work, gy.shape[0], n_out)
        return gx, gw, gb


def _train_linear(x, w, b):
    """F.linear(x, w, b) of the training forward: the split weight gradient (_SplitKLinear) when x
    has many rows (grad enabled, on the GPU), _LinearBG for short 2-D fp16 ones, plain autocast F.linear
    otherwise."""
    rows = x.numel() // x.shape[-1]
    if hip_training(x):
        if rows >= _SplitKLinear.MIN_ROWS and rows % _SplitKLinear.SPLIT == 0 and w.requires_grad:
            return _SplitKLinear.apply(x, w, b)
        if (x.dim() == 2 and x.dtype == w.dtype == torch.float16 and b is not None and
                b.dtype == torch.float16 and w.shape[0] % 8 == 0 and 0 < rows <= 8192 and x.stride(1) == 1):
            return _LinearBG.apply(x, w, b)
    return F.linear(x, w, b)
