"""Padded flow passes of CosyVoice-300M's U-Net estimator (csrc/flow.hip unet1_forward with a level-length table, cv_flow_solve_ragged, EstimatorHandle.solve_batch,
MaskedDiffWithXvec.inference_batch, CosyVoiceModel.tts_batch(flow_batch=...)).  The estimator is not causal and the reference's own padded form (flow/decoder.py:210-291)
does not reproduce its batch-1 result (its GroupNorm averages over the padding), so the yardstick is the project's own batch-1 path - pinned to the real classes by
tests/golden/cv1k_*.npz - and the contract is the one of cv_flow_estimator_masked: a row's valid frames come out as for that row alone at its own length, padded frames
are zero.  Every comparison below is torch.equal, in both precisions; no kernel form had to be excepted."""
import ctypes as C

import pytest
import torch

from cosyvoice_amd import cosyvoice1_hip as CK
from cosyvoice_amd import synthetic as W
from cv1k_common import CFG, build_flow, build_hift, gold

PRECISIONS = ["fp32", "bf16"]
LENS = (261, 130, 37, 2)         # 261 against 130: different GroupNorm slice counts at C = 32 (S = ceil(T / 256)); odd lengths: the stride-2 / transposed-convolution
                                 # edges; the even ones: the exact cut; 2 frames: 1 at the halved level
_handles = {}


def _handle(lib, precision):
    key = (id(lib), precision)
    if key not in _handles:
        _handles[key] = CK.EstimatorHandle(W.make_cv1_flow(CFG), "decoder.estimator.", CFG.est_heads, lib, precision)
    return _handles[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lens", [(261, 130), (37, 2)])
def test_estimator_padded_rows_equal_the_rows_alone(lib, precision, lens):
    """cv_flow_estimator_masked on the U-Net handle, two rows of different lengths padded to the longer: each row's valid frames equal EstimatorHandle.forward of that
    row alone at its own length, the padded frames are exactly zero.  The inputs are NOT zero behind a row's end: the entry point owes the contract to any input."""
    hd, T = _handle(lib, precision), max(lens)
    gen = torch.Generator().manual_seed(3 + T)
    x, mu, cond = (torch.randn(2, 80, T, generator=gen) for _ in range(3))
    spks, t = torch.randn(2, 80, generator=gen), torch.tensor([0.3, 0.8])
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).float().unsqueeze(1)
    got = hd.forward(x, mask, mu, t, spks, cond).cpu()
    for b, L in enumerate(lens):
        two = lambda a: torch.stack([a[b], a[b]])
        alone = hd.forward(two(x)[:, :, :L], torch.ones(2, 1, L), two(mu)[:, :, :L], two(t), two(spks), two(cond)[:, :, :L]).cpu()[0]
        assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
        assert torch.equal(got[b, :, :L], alone), (precision, lens, b, float((got[b, :, :L] - alone).abs().max()))
        assert L == T or float(got[b, :, L:].abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="ones for its valid frames"):
        hd.forward(x, 1 - mask, mu, t, spks, cond)


def test_generic_group_norm_form_on_padded_rows(lib):
    """The GENERIC length-aware GroupNorm (group_stats_kernel / group_apply_kernel, LEN instantiation) through cv_flow_estimator_masked: the U-Net's own widths (C / 4 a
    power of two) send every GroupNorm through the row-wise form, so this handle is 96 channels wide, the narrowest the generic form takes (C % 32 == 0 and C / 4 = 24
    does not divide 256).  A group is cg = 12 channels and its slice count ceil(len * 12 / 8192): row 0's 700 frames make two slices (8400 elements), row 1's single
    frame one - the rows of one launch differ in their slice count and the short row's second slice must do nothing.  Same contract and same equalities as above:
    a row's valid frames are those of the row alone at its own length, the frames behind them exact zeros."""
    import dataclasses
    cfg = dataclasses.replace(CFG, est_ch=[96], est_mid=1)                  # (one level, one mid block: the arm under test needs no more)
    hd = CK.EstimatorHandle(W.make_cv1_flow(cfg), "decoder.estimator.", cfg.est_heads, lib, "fp32")
    lens = (700, 1)
    T = max(lens)
    gen = torch.Generator().manual_seed(5)
    x, mu, cond = (torch.randn(2, 80, T, generator=gen) for _ in range(3))
    spks, t = torch.randn(2, 80, generator=gen), torch.tensor([0.3, 0.8])
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).float().unsqueeze(1)
    got = hd.forward(x, mask, mu, t, spks, cond).cpu()
    for b, L in enumerate(lens):
        two = lambda a: torch.stack([a[b], a[b]])
        alone = hd.forward(two(x)[:, :, :L], torch.ones(2, 1, L), two(mu)[:, :, :L], two(t), two(spks), two(cond)[:, :, :L]).cpu()[0]
        assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
        assert torch.equal(got[b, :, :L], alone), (b, float((got[b, :, :L] - alone).abs().max()))
        assert L == T or float(got[b, :, L:].abs().max()) == 0.0


def _solve_inputs(hd, lens, seed=17):
    gen = torch.Generator().manual_seed(seed)
    put = lambda a: hd.lib.hook(a.to(hd.dev).contiguous())
    return [tuple(put(torch.randn(L, 80, generator=gen)) for _ in range(3)) + (put(torch.randn(1, 80, generator=gen)),) for L in lens]      # (z, mu, cond, spk)


def _solve_batch(hd, reqs, order, n_steps):
    lens = [reqs[i][0].shape[0] for i in order]
    n, Tmax = len(order), max(lens)
    put = lambda a: hd.lib.hook(a.to(hd.dev).contiguous())
    x, mu, cond = (put(torch.zeros(n, Tmax, 80)) for _ in range(3))
    spk = put(torch.zeros(n, 80))
    for k, i in enumerate(order):
        L = lens[k]
        x[k, :L], mu[k, :L], cond[k, :L], spk[k] = reqs[i][0], reqs[i][1], reqs[i][2], reqs[i][3][0]
    hd.solve_batch(x, mu, spk, cond, lens, n_steps)
    for k, L in enumerate(lens):
        assert L == Tmax or float(x[k, L:].abs().max()) == 0.0       # the padded frames stay zero through every Euler step
    return {i: x[k, :lens[k]].cpu().clone() for k, i in enumerate(order)}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_solve_batch_equals_solve_alone(lib, precision):
    """solve_batch on four requests of lengths (261, 130, 37, 2): each equals `solve` alone on the same z / mu / spk / cond; again in reversed order (the position in the
    pass and the neighbour that sets Tmax do not matter); a one-request "batch" equals `solve`."""
    hd, n_steps = _handle(lib, precision), 2
    reqs = _solve_inputs(hd, LENS)
    alone = [hd.solve(z.clone(), mu, spk, cond, z.shape[0], n_steps).cpu() for z, mu, cond, spk in reqs]
    assert all(bool(torch.isfinite(a).all()) for a in alone) and len({a.shape[0] for a in alone}) == 4
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1]):
        got = _solve_batch(hd, reqs, order, n_steps)
        for i in order:
            assert torch.equal(got[i], alone[i]), (precision, order, i, float((got[i] - alone[i]).abs().max()))


def _seeded_noise(flow):
    """_draw_noise as a function of T only: both sides of a comparison see the same z whatever else drew from the host RNG."""
    flow._draw_noise = lambda T: torch.randn(1, 80, T, generator=torch.Generator().manual_seed(1000 + T))


def _flow_items():
    g = gold("cv1k_flow")
    gen = torch.Generator().manual_seed(41)
    tok = lambda n: torch.randint(0, CFG.speech_token_size, (1, n), generator=gen, dtype=torch.int32)
    e0, f0 = torch.zeros(1, 0, dtype=torch.int32), torch.zeros(1, 0, 80)
    n_p = int(g["prompt_token"].shape[1])
    return [dict(token=tok(45), prompt_token=e0, prompt_feat=f0, embedding=torch.randn(1, CFG.spk_dim, generator=gen)),             # > 40 tokens: head / middle / tail
            dict(token=tok(9), prompt_token=g["prompt_token"], prompt_feat=g["prompt_feat"], embedding=g["embedding"]),             # a prompt: tokens and frames
            dict(token=tok(17), prompt_token=e0, prompt_feat=f0, embedding=torch.randn(1, CFG.spk_dim, generator=gen))], n_p


@pytest.mark.parametrize("precision", PRECISIONS)
def test_inference_batch_equals_inference(lib, precision):
    """MaskedDiffWithXvec.inference_batch on three requests of different token counts (one with a prompt, one through the three-piece interpolation): each mel equals
    `inference` on that request alone; a non-empty flow cache and the "operators" estimator are errors."""
    flow = build_flow(lib, precision=precision)
    _seeded_noise(flow)
    flow.n_timesteps = 3                                            # (three Euler steps show what ten do: the emulator run stays short)
    items, n_p = _flow_items()
    t = lambda n: torch.tensor([n], dtype=torch.int32)
    empty = torch.zeros(1, 80, 0, 2)
    alone = [flow.inference(token=it["token"], token_len=t(it["token"].shape[1]), prompt_token=it["prompt_token"], prompt_token_len=t(it["prompt_token"].shape[1]),
                            prompt_feat=it["prompt_feat"], prompt_feat_len=t(it["prompt_feat"].shape[1]), embedding=it["embedding"], flow_cache=empty)[0].cpu() for it in items]
    got = [m.cpu() for m in flow.inference_batch(items)]
    assert n_p > 0 and len({a.shape[2] for a in alone}) == 3
    for a, b, it in zip(got, alone, items):
        assert b.shape == (1, 80, int(it["token"].shape[1] / CFG.input_frame_rate * 22050 / 256)) and bool(torch.isfinite(b).all())
        assert torch.equal(a, b), (precision, float((a - b).abs().max()))
    assert torch.equal(flow.inference_batch(items[2:])[0].cpu(), alone[2])
    with pytest.raises(ValueError, match="non-empty flow cache"):
        flow.inference_batch([dict(items[0], flow_cache=torch.zeros(1, 80, 34, 2)), items[1]])
    with pytest.raises(NotImplementedError, match="operators"):
        build_flow(lib, "operators").inference_batch(items[:2])


def test_tts_batch_shares_flow_passes(lib):
    """tts_batch(flow_batch=2) on three requests over two slots: every waveform equals `tts` of that request alone and tts_batch(flow_batch=1); at least one padded pass
    over two DIFFERENT lengths really ran (the solve_batch calls are counted); the per-uuid dicts are empty afterwards."""
    from test_zzz_cosyvoice1_hip_batch import _lm
    g = gold("cv1k_llm")
    gen = torch.Generator().manual_seed(9)
    m = CK.CosyVoiceModel(_lm(lib, sampling="greedy", decode_chunk=5), build_flow(lib), build_hift(lib))
    _seeded_noise(m.flow)
    m.flow.n_timesteps = 2                                          # (what is compared does not depend on the step count: two keep the emulator run short)
    rnd = lambda n, ratio: dict(text=torch.randint(0, CFG.text_vocab, (1, n), generator=gen, dtype=torch.int32), llm_embedding=torch.randn(1, CFG.spk_dim, generator=gen),
                                flow_embedding=torch.randn(1, CFG.spk_dim, generator=gen), max_token_text_ratio=ratio, min_token_text_ratio=ratio)
    reqs = [dict(text=g["text"][:, :4], llm_embedding=g["embedding"], flow_embedding=g["embedding"], max_token_text_ratio=2, min_token_text_ratio=2), rnd(4, 3), rnd(3, 3)]      # 8, 12 and 9 speech tokens
    hift_inf = m.hift.inference

    def seeded(**kw):
        torch.manual_seed(77)
        return hift_inf(**kw)
    m.hift.inference = seeded
    passes, solve_batch = [], m.flow.estimator.solve_batch

    def counted(x, mu, spk, cond, lens, n_steps):
        passes.append(list(lens))
        return solve_batch(x, mu, spk, cond, lens, n_steps)
    m.flow.estimator.solve_batch = counted
    inf = m.llm.inference
    alone = []
    for r in reqs:
        m.llm.inference = lambda _r=r, **kw: inf(**dict(kw, max_token_text_ratio=_r["max_token_text_ratio"], min_token_text_ratio=_r["min_token_text_ratio"]))
        alone.append(next(iter(m.tts(stream=False, **r)))["tts_speech"])
    m.llm.inference = inf
    assert not passes and len({a.shape[1] for a in alone}) == 3
    got = dict(m.tts_batch(reqs, slots=2, flow_batch=2, flow_pad=2.0))
    assert any(len(p) == 2 and p[0] != p[1] for p in passes), passes
    n_passes = len(passes)
    one = dict(m.tts_batch(reqs, slots=2, flow_batch=1))
    assert len(passes) == n_passes and sorted(got) == sorted(one) == [0, 1, 2]
    for i, want in enumerate(alone):
        assert float(want.abs().max()) > 0
        assert torch.equal(got[i]["tts_speech"], want) and torch.equal(one[i]["tts_speech"], want)
    assert not (m.tts_speech_token_dict or m.llm_end_dict or m.mel_overlap_dict or m.flow_cache_dict or m.hift_cache_dict)


def test_ragged_solve_entry_point_checks_its_arguments(emu_lib):
    """cv_flow_solve_ragged: a null pointer, a request count outside 1..8, a length outside 1..Tmax and a handle of another estimator are errors with a message, not
    aborts; cv_flow_inference and cv_flow_inference_ragged on the U-Net handle raise; the header declares the entry point and both libraries export it."""
    from cosyvoice_amd._lib import CosyVoiceAmdError
    from cosyvoice_amd.build import build_hip
    from cosyvoice_amd.flow import CausalMaskedDiffWithXvec
    from test_abi import declared_symbols
    hip = C.CDLL(build_hip())
    assert "cv_flow_solve_ragged" in declared_symbols() and hasattr(hip, "cv_flow_solve_ragged") and hasattr(emu_lib.dll, "cv_flow_solve_ragged")
    hd, i32 = _handle(emu_lib, "fp32"), C.c_int32
    buf = lambda *shape: emu_lib.hook(torch.zeros(*shape))
    x, mu, cond, spk = buf(2, 8, 80), buf(2, 8, 80), buf(2, 8, 80), buf(2, 80)
    p = lambda a: C.c_void_p(a.data_ptr())
    lens = lambda *v: (i32 * len(v))(*v)
    call = lambda h, n, xx, ll, Tmax=8, steps=1: emu_lib.cv_flow_solve_ragged(h, i32(n), xx, p(mu), p(spk), p(cond), ll, i32(Tmax), i32(steps), None)
    with pytest.raises(CosyVoiceAmdError, match="null argument"):
        call(hd._h, 2, None, lens(8, 3))
    with pytest.raises(CosyVoiceAmdError, match="null argument"):
        call(hd._h, 2, p(x), None)
    for n in (0, 9):
        with pytest.raises(CosyVoiceAmdError, match="1..8 utterances"):
            call(hd._h, n, p(x), lens(*([8] * 9)))
    for bad in ((8, 0), (9, 8), (-1, 8)):
        with pytest.raises(CosyVoiceAmdError, match="every length must be 1..Tmax"):
            call(hd._h, 2, p(x), lens(*bad))
    with pytest.raises(CosyVoiceAmdError, match="must be positive"):
        call(hd._h, 2, p(x), lens(8, 3), steps=0)
    call(hd._h, 2, p(x), lens(8, 3))                                 # (and the good call goes through: zero inputs, finite output, zeros behind the short row)
    assert bool(torch.isfinite(x).all()) and float(x[1, 3:].abs().max()) == 0.0
    lc, fc, hc = W.tiny()
    other = CausalMaskedDiffWithXvec(W.make_flow(fc), fc, lib=emu_lib)                  # (a handle of the causal CosyVoice2 estimator)
    with pytest.raises(CosyVoiceAmdError, match="estimator == 2"):
        call(other._h, 2, p(x), lens(8, 3))
    ids, out, n2 = emu_lib.hook(torch.zeros(8, dtype=torch.int32)), buf(80, 16), (i32 * 2)()
    with pytest.raises(CosyVoiceAmdError, match="holds no encoder"):
        emu_lib.cv_flow_inference(hd._h, p(ids), i32(8), None, i32(0), p(buf(192)), p(buf(16, 80)), i32(0), i32(1), i32(1), p(out), n2, None)
    with pytest.raises(CosyVoiceAmdError, match="holds no encoder"):
        emu_lib.cv_flow_inference_ragged(hd._h, i32(1), p(ids), lens(8), None, lens(0), p(buf(192)), p(buf(16, 80)), i32(0), i32(1), i32(1), p(out), n2, None)
