"""Operator-level parity: each HIP kernel vs a plain torch fp32 restatement of the same op."""
import math

import pytest
import torch
import torch.nn.functional as F

from cosyvoice_amd import ops


def _sync(lib):
    if not lib.emulated:
        torch.cuda.synchronize()


_LIB = {}


def _dev(lib):
    _LIB["lib"] = lib
    return torch.device(lib.device)


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return _LIB["lib"].hook((torch.randn(shape, generator=g) * scale).to(dev))


@pytest.mark.parametrize("M,N,K,wdt", [(5, 7, 9, torch.float32), (37, 48, 64, torch.bfloat16), (130, 200, 96, torch.bfloat16),
                                       (64, 64, 544, torch.float32)])
def test_linear(lib, M, N, K, wdt):
    dev = _dev(lib)
    A = _rand((M, K), dev, 1)
    W = _rand((N, K), dev, 2, 0.2).to(wdt).float()
    b = _rand((N,), dev, 3)
    Wp, Kp = ops.pack_weight(W, wdt)
    res = _rand((M, N), dev, 4)
    out = ops.gemm_conv(lib, A, Wp, Kp, M=M, N=N, K=K, bias=b, act="silu", res=res.reshape(1, M, N), out_scale=0.5)
    _sync(lib)
    ref = (F.silu(A @ W.t() + b) + res) * 0.5
    torch.testing.assert_close(out[0].cpu(), ref.cpu(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("N,K,act", [(7, 36, "none"), (1030, 1024, "relu"), (200, 4096, "silu"), (64, 96, "none")])
def test_single_row_gemv_fp32_weights(lib, N, K, act, monkeypatch):
    """Round 4: one output row over fp32 weights goes to gemv_f32_kernel (the decode step of CosyVoice-300M's LM) instead of a GEMM tile with one useful row -
    same epilogue contract as the tiled kernel ((act(x W^T + b) + res) * out_scale), K not a multiple of the 64-float step, N not a multiple of a workgroup's
    4 rows, a row-pitched weight view; and the tiled kernel (cv_ops_set_option "gemv_f32" = 0; the environment variable CV_GEMV_F32 is only read once per process,
    so toggling IT here compared the GEMV with itself - ADVICE r5) agrees to fp32 rounding."""
    import ctypes as C
    dev = _dev(lib)
    A = _rand((1, K), dev, 11)
    W = _rand((N, K), dev, 12, 0.2)
    b, res = _rand((N,), dev, 13), _rand((1, N), dev, 14)
    Wp, Kp = ops.pack_weight(W, torch.float32)
    ref = {"none": lambda v: v, "relu": F.relu, "silu": F.silu}[act](A @ W.t() + b)
    ref = (ref + res) * 0.5
    outs = []
    try:
        for knob in (1, 0):
            lib.cv_ops_set_option(b"gemv_f32", C.c_int32(knob))
            out = ops.gemm_conv(lib, A, Wp, Kp, M=1, N=N, K=K, bias=b, act=act, res=res.reshape(1, 1, N), out_scale=0.5)
            _sync(lib)
            outs.append(out[0].cpu())
            torch.testing.assert_close(outs[-1], ref.cpu(), rtol=3e-5, atol=3e-5)
    finally:
        lib.cv_ops_set_option(b"gemv_f32", C.c_int32(1))
    torch.testing.assert_close(outs[0], outs[1], rtol=2e-5, atol=2e-5)
    if K >= 1024:
        assert not torch.equal(outs[0], outs[1])                    # two kernels, two summation orders: the knob really switched


@pytest.mark.parametrize("M,N,K,taps", [(37, 48, 64, 1), (130, 200, 96, 1), (300, 256, 1024, 1), (70, 96, 320, 3), (33, 40, 36, 1)])
def test_linear_bf16_mfma(lib, M, N, K, taps):
    """a_bf16 = 1: activations (after the fused input activation) are rounded to bf16 round-to-nearest-even and multiplied with
    the bf16 weights on v_mfma_f32_16x16x32_bf16, fp32 accumulate.  Reference = the same rounding done in torch; the products
    of two bf16 values are exact in fp32, so only the summation order differs."""
    dev = _dev(lib)
    x = _rand((M + taps - 1, K), dev, 11)                                     # causal conv over rows when taps > 1
    W = _rand((N, taps, K), dev, 12, 0.2).bfloat16().float()
    b = _rand((N,), dev, 13)
    Wp, Kp = ops.pack_weight(W if taps > 1 else W[:, 0], torch.bfloat16)
    out = ops.gemm_conv(lib, x, Wp, Kp, M=M, N=N, K=K, taps=taps, lda=K, tap_step=K, a_len=x.numel(), bias=b, pro="leaky", pro_p=0.1, act="gelu_erf", a_bf16=True)
    _sync(lib)
    xa = F.leaky_relu(x, 0.1).bfloat16().float()      # (a transcendental prologue could flip a bf16 rounding by its last-ulp difference)
    ref = sum(xa[j:j + M] @ W[:, j].t() for j in range(taps)) + b
    ref = F.gelu(ref)
    torch.testing.assert_close(out[0].cpu(), ref.cpu(), rtol=3e-5, atol=3e-5)
    exact = ops.gemm_conv(lib, x, Wp, Kp, M=M, N=N, K=K, taps=taps, lda=K, tap_step=K, a_len=x.numel(), bias=b, pro="leaky", pro_p=0.1, act="gelu_erf")
    _sync(lib)
    assert not torch.equal(exact, out)                                       # the flag really selects the other kernel
    torch.testing.assert_close(out[0].cpu(), exact[0].cpu(), rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("T,Cin,Cout,k,dil,causal", [(50, 16, 24, 3, 1, True), (70, 32, 32, 7, 3, False), (33, 80, 40, 11, 5, False)])
def test_conv1d(lib, T, Cin, Cout, k, dil, causal):
    """Conv1d on channel-last activations == torch conv1d on [B,C,T] (flow/decoder.py:36-62, hifigan/generator.py:46-122)."""
    dev = _dev(lib)
    B = 2
    x = _rand((B, T, Cin), dev, 5)                       # channel-last
    w = _rand((Cout, Cin, k), dev, 6, 0.2)
    b = _rand((Cout,), dev, 7)
    alpha = (_rand((Cin,), dev, 8).abs() + 0.5)
    pad_l = (k - 1) * dil if causal else (k * dil - dil) // 2
    Wp, Kp = ops.pack_weight(w.permute(0, 2, 1).contiguous(), torch.float32)     # [N, taps, Cin]
    alpha_p = torch.zeros(Kp, device=dev); alpha_p[:Cin] = alpha
    out = ops.gemm_conv(lib, x, Wp, Kp, M=T, N=Cout, K=Cin, taps=k, lda=Cin, a_off0=-pad_l * Cin, tap_step=dil * Cin,
                        a_len=T * Cin, a_batch=T * Cin, batch=B, c_batch=T * Cout, bias=b, pro="snake", pro_alpha=alpha_p)
    _sync(lib)
    xs = x.transpose(1, 2)
    xs = xs + (1.0 / (alpha[None, :, None] + 1e-9)) * torch.sin(xs * alpha[None, :, None]) ** 2
    if causal:
        ref = F.conv1d(F.pad(xs, (pad_l, 0)), w, b, dilation=dil)
    else:
        ref = F.conv1d(xs, w, b, dilation=dil, padding=pad_l)
    torch.testing.assert_close(out.cpu(), ref.transpose(1, 2).cpu(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("T,Cin,Cout,k,s,p", [(40, 18, 16, 30, 15, 7), (31, 18, 8, 6, 3, 1)])
def test_strided_conv(lib, T, Cin, Cout, k, s, p):
    """source_downs: Conv1d(18, C, k=2u, stride=u, padding=u//2) (hifigan/generator.py:449-451) as an im2col-free GEMM."""
    dev = _dev(lib)
    x = _rand((T, Cin), dev, 9)
    w = _rand((Cout, Cin, k), dev, 10, 0.2)
    b = _rand((Cout,), dev, 11)
    Tout = (T + 2 * p - k) // s + 1
    Wp, Kp = ops.pack_weight(w.permute(0, 2, 1).reshape(Cout, 1, k * Cin).contiguous(), torch.float32)
    out = ops.gemm_conv(lib, x, Wp, Kp, M=Tout, N=Cout, K=k * Cin, lda=s * Cin, a_off0=-p * Cin, a_len=T * Cin, bias=b)
    _sync(lib)
    ref = F.conv1d(x.t()[None], w, b, stride=s, padding=p)[0].t()
    torch.testing.assert_close(out[0].cpu(), ref.cpu(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("T,Cin,Cout,k,s", [(12, 32, 16, 16, 8), (9, 16, 8, 11, 5), (10, 8, 4, 7, 3)])
def test_conv_transpose(lib, T, Cin, Cout, k, s):
    """ConvTranspose1d(k, stride s, padding (k-s)//2) in polyphase form (hifigan/generator.py:428-441)."""
    dev = _dev(lib)
    p = (k - s) // 2
    x = _rand((T, Cin), dev, 12)
    w = _rand((Cin, Cout, k), dev, 13, 0.2)
    b = _rand((Cout,), dev, 14)
    Tout = (T - 1) * s - 2 * p + k
    q = (k + s - 1) // s
    wp = torch.zeros(s, Cout, q, Cin, device=dev)          # [(r, co), tap q, ci] = w[ci, co, r + s*q]
    for r in range(s):
        for qq in range(q):
            if r + s * qq < k:
                wp[r, :, qq, :] = w[:, :, r + s * qq].t()
    Wp, Kp = ops.pack_weight(wp.reshape(s * Cout, q, Cin), torch.float32)
    out = torch.zeros(1, Tout, Cout, device=dev)
    ops.gemm_conv(lib, x, Wp, Kp, M=T + q - 1, N=s * Cout, K=Cin, taps=q, lda=Cin, tap_step=-Cin, a_len=T * Cin,
                  bias=b.repeat(s), out=out, ldc=s * Cout, c_off=-p * Cout, c_len=Tout * Cout, pro="leaky", pro_p=0.1)
    _sync(lib)
    ref = F.conv_transpose1d(F.leaky_relu(x.t()[None], 0.1), w, b, stride=s, padding=p)[0].t()
    torch.testing.assert_close(out[0].cpu(), ref.cpu(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("rows,C,rms", [(7, 80, False), (9, 256, False), (5, 896, True), (3, 30, False)])
def test_norm_rows(lib, rows, C, rms):
    dev = _dev(lib)
    x = _rand((rows, C), dev, 15) * 3 + 1
    g = _rand((C,), dev, 16); b = _rand((C,), dev, 17)
    if rms:
        out = ops.norm_rows(lib, x, gamma=g, eps=1e-6, rms=True)
        ref = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * g
    else:
        rs = _rand((rows,), dev, 18); ca = _rand((1, C), dev, 19)
        out = ops.norm_rows(lib, x, gamma=g, beta=b, eps=1e-5, act="mish", scale=2.0, row_scale=rs, col_add=ca)
        ref = F.mish(F.layer_norm(x, (C,), g, b, 1e-5)) * 2.0 * rs[:, None] + ca
    _sync(lib)
    torch.testing.assert_close(out.cpu(), ref.cpu(), rtol=2e-5, atol=2e-5)


def _ref_attn(q, k, v, scale, mask):
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    s = s.masked_fill(~mask, float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)


@pytest.mark.parametrize("Tq,Tk,mode,chunk", [(70, 70, "none", 0), (50, 50, "chunk", 16), (33, 81, "causal", 0), (130, 130, "chunk", 50)])
def test_attention(lib, Tq, Tk, mode, chunk):
    dev = _dev(lib)
    B, H, G = 2, 4, 2
    qkv = _rand((B, Tq, 3 * H * 64), dev, 20)                 # fused-QKV row layout as the flow estimator produces it
    q = qkv[..., :H * 64].view(B, Tq, H, 64)
    if Tk == Tq:
        k = qkv[..., H * 64:2 * H * 64].view(B, Tq, H, 64); v = qkv[..., 2 * H * 64:].view(B, Tq, H, 64); group = 1
    else:   # GQA against a cache laid out [B, Hkv, Tk, 64]
        kc = _rand((B, H // G, Tk, 64), dev, 21); vc = _rand((B, H // G, Tk, 64), dev, 22)
        k = kc.permute(0, 2, 1, 3); v = vc.permute(0, 2, 1, 3); group = G
    scale = 1 / 8.0
    out = ops.attention(lib, q, k, v, scale=scale, mask=mode, chunk=chunk, kv_group=group)
    _sync(lib)
    qi = torch.arange(Tq)[:, None]; kj = torch.arange(Tk)[None, :]
    if mode == "none":
        m = torch.ones(Tq, Tk, dtype=torch.bool)
    elif mode == "causal":
        m = kj <= qi + (Tk - Tq)
    else:
        m = kj < (qi // chunk + 1) * chunk
    kk = k.repeat_interleave(group, dim=2) if group > 1 else k
    vv = v.repeat_interleave(group, dim=2) if group > 1 else v
    ref = _ref_attn(q.cpu(), kk.cpu(), vv.cpu(), scale, m[None, None])
    torch.testing.assert_close(out.cpu(), ref, rtol=2e-5, atol=2e-5)


def test_attention_relpos(lib):
    """scores = (ac + rel_shift(bd)) / sqrt(d)  (cosyvoice/transformer/attention.py:222-244,318-326)."""
    dev = _dev(lib)
    B, H, T = 1, 2, 37
    q = _rand((B, T, H, 64), dev, 23); k = _rand((B, T, H, 64), dev, 24); v = _rand((B, T, H, 64), dev, 25)
    bd = _rand((B, H, T, 2 * T - 1), dev, 26)
    out = ops.attention(lib, q, k, v, scale=1 / 8.0, rel_bd=bd)
    _sync(lib)
    x = bd.cpu()
    zero_pad = torch.zeros((B, H, T, 1))
    x_padded = torch.cat([zero_pad, x], dim=-1).view(B, H, 2 * T, T)
    shifted = x_padded[:, :, 1:].view_as(x)[:, :, :, :T]
    s = (torch.einsum("bqhd,bkhd->bhqk", q.cpu(), k.cpu()) + shifted) / 8.0
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.cpu())
    torch.testing.assert_close(out.cpu(), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("variant", [2, 3])      # 2: 64-query workgroups (two tiles in flight), 3: 32-query workgroups (co-resident)
@pytest.mark.parametrize("Tq,Tk,mode,chunk", [(70, 70, "none", 0), (50, 50, "chunk", 16), (33, 81, "causal", 0), (200, 200, "chunk", 50), (300, 300, "none", 0)])
def test_attention_bf16_mfma(lib, Tq, Tk, mode, chunk, variant):
    """bf16 = 1: q, k, v rounded to bf16 (products exact in fp32), probabilities rounded to bf16 for the P.V product only
    (the denominator sums the unrounded ones).  Reference: the same operand rounding in torch with fp32 probabilities; what is
    left is the bf16 rounding of P, relative 2^-9 per term and averaging out over the keys: tolerance 4e-3 on O(1) outputs."""
    dev = _dev(lib)
    B, H, G = 2, 4, 2
    qkv = _rand((B, Tq, 3 * H * 64), dev, 20)
    q = qkv[..., :H * 64].view(B, Tq, H, 64)
    if Tk == Tq:
        k = qkv[..., H * 64:2 * H * 64].view(B, Tq, H, 64); v = qkv[..., 2 * H * 64:].view(B, Tq, H, 64); group = 1
    else:
        kc = _rand((B, H // G, Tk, 64), dev, 21); vc = _rand((B, H // G, Tk, 64), dev, 22)
        k = kc.permute(0, 2, 1, 3); v = vc.permute(0, 2, 1, 3); group = G
    out = ops.attention(lib, q, k, v, scale=1 / 8.0, mask=mode, chunk=chunk, kv_group=group, bf16=variant)
    auto = ops.attention(lib, q, k, v, scale=1 / 8.0, mask=mode, chunk=chunk, kv_group=group, bf16=True)
    exact = ops.attention(lib, q, k, v, scale=1 / 8.0, mask=mode, chunk=chunk, kv_group=group)
    _sync(lib)
    qi = torch.arange(Tq)[:, None]; kj = torch.arange(Tk)[None, :]
    m = torch.ones(Tq, Tk, dtype=torch.bool) if mode == "none" else (kj <= qi + (Tk - Tq) if mode == "causal" else kj < (qi // chunk + 1) * chunk)
    kk = k.repeat_interleave(group, dim=2) if group > 1 else k
    vv = v.repeat_interleave(group, dim=2) if group > 1 else v
    r = lambda t: t.cpu().bfloat16().float()
    ref = _ref_attn(r(q), r(kk), r(vv), 1 / 8.0, m[None, None])
    torch.testing.assert_close(out.cpu(), ref, rtol=4e-3, atol=4e-3)
    assert not torch.equal(out, exact)
    torch.testing.assert_close(out.cpu(), exact.cpu(), rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(auto.cpu(), ref, rtol=4e-3, atol=4e-3)          # bf16=1 picks one of the two variants


def test_attention_relpos_bf16_mfma(lib):
    dev = _dev(lib)
    B, H, T = 1, 2, 90
    q = _rand((B, T, H, 64), dev, 23); k = _rand((B, T, H, 64), dev, 24); v = _rand((B, T, H, 64), dev, 25)
    bd = _rand((B, H, T, 2 * T - 1), dev, 26)
    out = ops.attention(lib, q, k, v, scale=1 / 8.0, rel_bd=bd, bf16=True)
    _sync(lib)
    x = bd.cpu()
    x_padded = torch.cat([torch.zeros((B, H, T, 1)), x], dim=-1).view(B, H, 2 * T, T)
    shifted = x_padded[:, :, 1:].view_as(x)[:, :, :, :T]
    r = lambda t: t.cpu().bfloat16().float()
    s = (torch.einsum("bqhd,bkhd->bhqk", r(q), r(k)) + shifted) / 8.0
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), r(v))
    torch.testing.assert_close(out.cpu(), ref, rtol=4e-3, atol=4e-3)


@pytest.mark.parametrize("act,ref", [("silu", F.silu), ("gelu_erf", F.gelu), ("mish", F.mish), ("tanh", torch.tanh), ("elu", F.elu)])
def test_activations(lib, act, ref):
    """Epilogue activations on the hardware transcendentals (common.h): |err| <= 3e-7 * max(1, |x|) against torch's libm forms,
    over [-30, 30] including the saturated tails.  Driven through the GEMM epilogue with an exact identity weight (fp32)."""
    dev = _dev(lib)
    n = 64
    x = torch.cat([torch.linspace(-30, 30, 40 * n - 4 * n), torch.linspace(-1e-3, 1e-3, 4 * n)]).reshape(-1, n)
    xd = lib.hook(x.to(dev).contiguous())
    Wp, Kp = ops.pack_weight(torch.eye(n, device=dev), torch.float32)
    out = ops.gemm_conv(lib, xd, Wp, Kp, M=x.shape[0], N=n, K=n, act=act)
    _sync(lib)
    want = ref(x)
    err = (out[0].cpu() - want).abs()
    bound = 3e-7 * torch.clamp(x.abs(), min=1.0)
    assert bool((err <= bound).all()), (act, err.max().item(), x.flatten()[err.argmax()].item())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5])
def test_every_gemm_tile_shape(lib, tile, bf16, monkeypatch):
    """The tile shape is chosen from the launch size (gemm_conv.hip), so small problems only ever meet the smallest one.
    CV_GEMM_FORCE_TILE pins it: every instantiation (128x128 .. 32x32, and the two-wave 16x32 of the bf16 path), both K depths, with
    ragged M / N / K edges, a causal 3-tap conv window, bias + residual epilogue, against torch."""
    if tile == 5 and not bf16:
        pytest.skip("the 16x32 two-wave tile exists for the bf16 path only")
    dev = _dev(lib)
    monkeypatch.setenv("CV_GEMM_FORCE_TILE", str(tile))
    for (M, N, K, taps) in [(150, 140, 160, 1), (70, 200, 36, 3), (40, 33, 320, 1)]:
        if tile == 5 and K < 97:
            continue                                                  # (Kp >= 128 is required for that tile)
        x = _rand((M + taps - 1, K), dev, 31)
        W = _rand((N, taps, K), dev, 32, 0.2).bfloat16().float()
        b = _rand((N,), dev, 33); res = _rand((M, N), dev, 34)
        Wp, Kp = ops.pack_weight(W if taps > 1 else W[:, 0], torch.bfloat16)
        out = ops.gemm_conv(lib, x, Wp, Kp, M=M, N=N, K=K, taps=taps, lda=K, tap_step=K, a_len=x.numel(), bias=b, res=res.reshape(1, M, N), a_bf16=bf16)
        _sync(lib)
        xa = x.bfloat16().float() if bf16 else x
        ref = sum(xa[j:j + M] @ W[:, j].t() for j in range(taps)) + b + res
        torch.testing.assert_close(out[0].cpu(), ref.cpu(), rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_two_sided_split_fp32_weights(lib, tile, monkeypatch):
    """fp32 activations x fp32 WEIGHTS (HiFT): both operands split into three bf16 planes (weights at load time, weights.split3_planes; activations
    when staged), six exact plane products per k on v_mfma_f32_16x16x32_bf16 (gemm_conv.h WX3) against a float64 reference and against the fp32 MFMA
    chain (CV_GEMM_WX3=0).  The dropped products are below one fp32 rounding of a term, so both stay at fp32-accumulation distance from float64.  Every
    tile shape, ragged M / N / K edges, a dilated 3-tap "same" window, Snake prologue + bias + residual epilogue (a HiFT ResBlock convolution)."""
    from cosyvoice_amd.weights import split3_planes
    dev = _dev(lib)
    monkeypatch.setenv("CV_GEMM_FORCE_TILE", str(tile))
    for (M, N, K, taps, dil) in [(150, 140, 160, 1, 1), (90, 64, 64, 3, 3), (40, 33, 320, 1, 1)]:
        rows = M + (taps - 1) * dil
        x = _rand((rows, K), dev, 41, 2.0)
        W = _rand((N, taps, K), dev, 42, 0.2)                       # full fp32 mantissas
        W[0, 0, :4] = torch.tensor([1.0 + 2.0 ** -20, 3.0e-7, -1.0 - 2.0 ** -23, 0.0])      # values whose low planes matter
        b = _rand((N,), dev, 43); res = _rand((M, N), dev, 44)
        Wp, Kp = ops.pack_weight(W if taps > 1 else W[:, 0], torch.float32)
        W3 = lib.hook(split3_planes(Wp))
        assert torch.equal(W3.float().reshape(N, 3, -1).sum(1), Wp)                      # w1 + w2 + w3 == w exactly
        alpha = lib.hook(torch.ones(Kp, device=dev) + 0.3 * _rand((Kp,), dev, 45).abs())
        kw = dict(M=M, N=N, K=K, taps=taps, lda=K, tap_step=dil * K, a_len=x.numel(), bias=b, res=res.reshape(1, M, N), pro="snake", pro_alpha=alpha)
        monkeypatch.delenv("CV_GEMM_WX3", raising=False)
        split = ops.gemm_conv(lib, x, Wp, Kp, w3=W3, **kw)[0].cpu().double(); _sync(lib)
        monkeypatch.setenv("CV_GEMM_WX3", "0")
        chain = ops.gemm_conv(lib, x, Wp, Kp, w3=W3, **kw)[0].cpu().double(); _sync(lib)
        a = alpha.cpu().double()[:K]
        xs = x.cpu().double(); xs = xs + torch.sin(xs * a) ** 2 / (a + 1e-9)
        ref = sum(xs[j * dil:j * dil + M] @ W.cpu().double()[:, j].t() for j in range(taps)) + b.cpu().double() + res.cpu().double()
        scale = ref.abs().max().item()
        e_split, e_chain = (split - ref).abs().max().item() / scale, (chain - ref).abs().max().item() / scale
        assert not torch.equal(split, chain) or lib.emulated is None
        assert e_split < 3e-6 and e_chain < 3e-6 and e_split < 4 * e_chain + 2e-7, (tile, M, N, K, e_split, e_chain)


@pytest.mark.parametrize("M,N,K,taps", [(37, 48, 64, 1), (131, 200, 896, 1), (70, 96, 320, 3)])
def test_linear_three_term_split_is_fp32_exact(lib, M, N, K, taps, monkeypatch):
    """fp32 activations x bf16 weights: the three-term bf16 split on v_mfma_f32_16x16x32_bf16 (gemm_conv.h AX3, the default) against a float64
    reference and against the fp32 MFMA chain (CV_GEMM_X3=0, read at every launch).  The split is exact (x1 + x2 + x3 == x, every product exact),
    so both differ from float64 only by fp32 accumulation: errors of the same size, far below the bf16-activation mode's."""
    dev = _dev(lib)
    x = _rand((M + taps - 1, K), dev, 21, 3.0)
    W = _rand((N, taps, K), dev, 22, 0.2).bfloat16().float()
    Wp, Kp = ops.pack_weight(W if taps > 1 else W[:, 0], torch.bfloat16)
    run = lambda: ops.gemm_conv(lib, x, Wp, Kp, M=M, N=N, K=K, taps=taps, lda=K, tap_step=K, a_len=x.numel())[0].cpu().double()
    monkeypatch.delenv("CV_GEMM_X3", raising=False)
    split = run(); _sync(lib)
    monkeypatch.setenv("CV_GEMM_X3", "0")
    chain = run(); _sync(lib)
    ref = sum(x.cpu().double()[j:j + M] @ W.cpu().double()[:, j].t() for j in range(taps))
    scale = ref.abs().max().item()
    e_split, e_chain = (split - ref).abs().max().item() / scale, (chain - ref).abs().max().item() / scale
    assert e_split < 2e-6 and e_chain < 2e-6 and e_split < 4 * e_chain + 1e-7, (e_split, e_chain)
    # the three planes really carry the whole fp32 value: activations with a tiny component next to a large one keep it
    y = x.clone(); y[:, 0] = 1000.0; y[:, 1] = 1e-3
    out = ops.gemm_conv(lib, y, Wp, Kp, M=M, N=N, K=K, taps=taps, lda=K, tap_step=K, a_len=y.numel())[0].cpu().double()
    refy = sum(y.cpu().double()[j:j + M] @ W.cpu().double()[:, j].t() for j in range(taps))
    assert (out - refy).abs().max().item() / refy.abs().max().item() < 2e-6


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode,chunk", [("none", 0), ("chunk", 16)])
def test_attention_key_counts_per_batch_row(lib, bf16, mode, chunk):
    """cv_attn_args.klen: in a padded batch, row b attends only its own klen[b] keys - and its valid queries get EXACTLY (bit for bit) what the same
    row gets alone in a batch of its own length: the key loop ends where it ends for the row alone."""
    dev = _dev(lib)
    B, H, T = 3, 2, 150
    lens = [150, 97, 33]
    q = _rand((B, T, H, 64), dev, 31); k = _rand((B, T, H, 64), dev, 32); v = _rand((B, T, H, 64), dev, 33)
    klen = lib.hook(torch.tensor(lens, dtype=torch.int32).to(dev))
    got = ops.attention(lib, q, k, v, scale=0.125, mask=mode, chunk=chunk, bf16=bf16, klen=klen)
    _sync(lib)
    for b, n in enumerate(lens):
        alone = ops.attention(lib, lib.hook(q[b:b + 1, :n].contiguous()), lib.hook(k[b:b + 1, :n].contiguous()), lib.hook(v[b:b + 1, :n].contiguous()),
                              scale=0.125, mask=mode, chunk=chunk, bf16=bf16)
        _sync(lib)
        assert torch.equal(got[b, :n].cpu(), alone[0].cpu())
        assert bool(torch.isfinite(got[b]).all())


# ---- peaky scores against a float64 reference (the constructions of test_flow_attention.py): attention_kernel (fp32) and attention_bf16_kernel (variants 2, 3)

def _attn64(q, k, v, scale, chunk, klen):
    """float64 attention with the klen / chunk mask -> (out [B, T, H, 64], vmax [B, T, H] = max |v| over the keys a query sees)."""
    B, T, H, _ = q.shape
    out = torch.zeros(B, T, H, 64, dtype=torch.float64); vmax = torch.zeros(B, T, H, dtype=torch.float64)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    for b in range(B):
        vis = j < klen[b]
        if chunk > 0:
            vis = vis & (j < (i // chunk + 1) * chunk)
        s = (torch.einsum("qhd,khd->hqk", q[b].double(), k[b].double()) * scale).masked_fill(~vis[None], float("-inf"))
        out[b] = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v[b].double())
        vmax[b] = torch.where(vis[:, :, None], v[b].double().abs().amax(-1)[None], torch.zeros(())).amax(1)
    return out, vmax


def _check_attn64(out, q, k, v, scale, chunk, klen, bf16):
    """bf16 (q, k, v already rounded to bf16, the kernel's exact operands): P is rounded to bf16 for P.V (relative 2^-8 per probability) while the
    denominator sums the unrounded P, the output stays fp32 -> |o - ref| <= 2^-8 vmax (1 + 2^-5).  fp32: a score is a 64-term fp32 dot product, absolute
    error <= 64 2^-24 scale max sum_d |q_d k_d| = delta, which moves every probability by a relative exp(2 delta) - 1 ~ 2 delta, then fp32 rounding of the sums:
    |o - ref| <= (2 delta + 2^-18) (vmax + |ref|)."""
    ref, vmax = _attn64(q, k, v, scale, chunk, klen)
    err = (out.cpu().double() - ref).abs()
    if bf16:
        bound = 2.0 ** -8 * vmax[..., None] * (1 + 2.0 ** -5)
    else:
        delta = 64 * 2.0 ** -24 * scale * torch.einsum("bqhd,bkhd->bhqk", q.abs().double(), k.abs().double()).max().item()
        bound = (2 * delta + 2.0 ** -18) * (vmax[..., None] + ref.abs())
    assert bool((err <= bound).all()), (err.max().item(), (err / bound).max().item())


def _growing_keys(B, T, H, seed):
    """Scores along one direction: q = (8 sigma, noise), k = (level / 8, noise), sigma alternating query by query.  Levels: tile 0 (keys 0-63) at 0, then a plateau
    at 44 with a spike of 48 in tile 1 and one of 96 in tile 3 - the running maximum of a sigma = +1 query jumps twice after tile 0 while plateau keys from
    before the second jump keep ~14 % of the weight (V mean +2 on tiles 1-2, -2 after them): a rescale that forgets the denominator, the accumulators or
    the new maximum is off by a large fraction of vmax.  sigma = -1 queries see the mirror image (their maximum never moves after tile 0)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H, 64, generator=g) * 0.2; k = torch.randn(B, T, H, 64, generator=g) * 0.2; v = torch.randn(B, T, H, 64, generator=g) * 0.5
    levels = torch.full((T,), 44.0); levels[:64] = 0.0; levels[64 + 5] = 48.0; levels[192 + 17] = 96.0
    q[..., 0] = 8.0 * (1.0 - 2.0 * (torch.arange(T) % 2).float())[None, :, None]
    k[..., 0] = (levels / 8.0)[None, :, None]
    v[:, 64:192] += 2.0; v[:, 192:] -= 2.0
    return q, k, v


@pytest.mark.parametrize("bf16", [False, 2, 3])
@pytest.mark.parametrize("chunk", [0, 100])
def test_attention_growing_key_norms_fp64(lib, bf16, chunk):
    """attention_kernel / attention_bf16_kernel (the conformer encoder, the CosyVoice3 DiT, prefill) on scores whose running maximum jumps by ~50 raw units twice
    after the first key tile (random inputs give a spread of ~8): the online-softmax rescale with live accumulators, against float64, with klen and the chunk mask."""
    dev = _dev(lib)
    B, T, H = 2, 320, 2
    q, k, v = _growing_keys(B, T, H, 71)
    if bf16:
        q, k, v = q.bfloat16().float(), k.bfloat16().float(), v.bfloat16().float()
    klen = [T, 250]
    kl = lib.hook(torch.tensor(klen, dtype=torch.int32).to(dev))
    out = ops.attention(lib, lib.hook(q.to(dev)), lib.hook(k.to(dev)), lib.hook(v.to(dev)), scale=0.125, mask="chunk" if chunk else "none", chunk=chunk, bf16=bf16, klen=kl)
    _sync(lib)
    _check_attn64(out, q, k, v, 0.125, chunk, klen, bf16)


@pytest.mark.parametrize("bf16", [False, 2, 3])
@pytest.mark.parametrize("chunk", [0, 13, 50])
def test_attention_dominant_masked_keys_fp64(lib, bf16, chunk):
    """Masked keys that would dominate if seen: K rows at or past klen[b] score +200 against every query (V there 3e4) - the output bits equal those of a launch
    with zeros there; chunk edges: the first and the last key of every chunk score +22 (x16 weight) with V = +3 / -3, so a query that sees one key past its chunk or
    misses its chunk's last one is off by far more than the float64 bound.  klen 150 / 97 / 33 / 1 (T = 150), chunks 13 (several boundaries per 64-query workgroup) and 50."""
    dev = _dev(lib)
    B, T, H = 4, 150, 2
    klen = [150, 97, 33, 1]
    g = torch.Generator().manual_seed(72 + chunk)
    q = torch.randn(B, T, H, 64, generator=g) * 0.5; k = torch.randn(B, T, H, 64, generator=g) * 0.5; v = torch.randn(B, T, H, 64, generator=g)
    q[..., 0] = 1.0
    j = torch.arange(T)
    c = chunk if chunk > 0 else T
    first, last = (j % c == 0), (j % c == c - 1)
    k[:, first, :, 0] = 22.0; k[:, last, :, 0] = 22.0
    v[:, first] = 3.0 + 0.1 * v[:, first]; v[:, last] = -3.0 + 0.1 * v[:, last]
    kz, vz, kf, vf = k.clone(), v.clone(), k.clone(), v.clone()
    for b, n in enumerate(klen):
        kz[b, n:] = 0.0; vz[b, n:] = 0.0
        kf[b, n:] = 4.0; kf[b, n:, :, 0] = 200.0; vf[b, n:] = 3.0e4
    if bf16:
        q, kz, vz, kf, vf = (t.bfloat16().float() for t in (q, kz, vz, kf, vf))
    kl = lib.hook(torch.tensor(klen, dtype=torch.int32).to(dev))
    mode = "chunk" if chunk else "none"
    outs = []
    for kk, vv in ((kf, vf), (kz, vz)):
        outs.append(ops.attention(lib, lib.hook(q.to(dev)), lib.hook(kk.to(dev)), lib.hook(vv.to(dev)), scale=0.125, mask=mode, chunk=chunk, bf16=bf16, klen=kl))
        _sync(lib)
    assert torch.equal(outs[0].cpu(), outs[1].cpu()), "masked keys changed the output"
    _check_attn64(outs[1], q, kz, vz, 0.125, chunk, klen, bf16)
