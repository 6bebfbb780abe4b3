"""Lock-step batched decode of CosyVoice-300M's TransformerLM (csrc/lm1.hip cv_lm1_batch_*, TransformerLM.inference_batch, CosyVoiceModel.tts_batch).  The reference
has no batched form (llm/llm.py:162-223 is batch-1): the yardstick is the project's own single-sequence path, itself pinned to the real class by tests/golden/cv1k_llm.npz.
The batched GEMVs keep, per slot, the products and the summation order of the single-sequence kernels, so every comparison below is an EQUALITY of bits or of token ids."""
import ctypes as C
import dataclasses

import pytest
import torch

from cosyvoice_amd import cosyvoice1_hip as CK
from cosyvoice_amd import synthetic as W
from cosyvoice_amd.llm import SamplingC
from cv1k_common import CFG, build_flow, build_hift, gold, t

MID = dataclasses.replace(CFG, llm_dim=512, text_heads=8, text_ffn=128, text_blocks=1, llm_heads=8, llm_ffn=1280, llm_blocks=2)     # test_wide_bf16_gemv_kernels_at_a_middle_size
E0 = torch.zeros(1, 0, dtype=torch.int32)


def _requests():
    g = gold("cv1k_llm")
    kw = dict(text=g["text"], text_len=t(7), prompt_text=g["prompt_text"], prompt_text_len=t(4), prompt_speech_token=g["prompt_speech_token"],
              prompt_speech_token_len=t(9), embedding=g["embedding"], max_token_text_ratio=6, min_token_text_ratio=2)
    sft = dict(kw, prompt_text=E0, prompt_text_len=t(0), prompt_speech_token=E0, prompt_speech_token_len=t(0), max_token_text_ratio=5)
    return g, kw, sft


def _five(cfg=CFG):
    """Five inference_sft-shaped requests of differing text lengths and token budgets."""
    gen = torch.Generator().manual_seed(31)
    out = []
    for n, hi, lo in ((3, 4, 2), (7, 3, 1), (5, 2, 2), (4, 5, 3), (6, 1, 0)):
        text = torch.randint(0, cfg.text_vocab, (1, n), generator=gen, dtype=torch.int32)
        out.append(dict(text=text, text_len=t(n), prompt_text=E0, prompt_text_len=t(0), prompt_speech_token=E0, prompt_speech_token_len=t(0),
                        embedding=torch.randn(1, cfg.spk_dim, generator=gen), max_token_text_ratio=hi, min_token_text_ratio=lo))
    return out


def _collect(gen, n):
    got = [[] for _ in range(n)]
    for i, toks in gen:
        got[i] += toks
    return got


def _lm(lib, cfg=CFG, **kw):
    return CK.TransformerLM(W.make_cv1_llm(cfg), text_heads=cfg.text_heads, llm_heads=cfg.llm_heads, lib=lib, **kw)


class _Seqs:
    """Sequences for the step-level tests: a random prompt per sequence (prefilled through forward_chunk), a random first input row, then the embedding row of the token
    the greedy sampler picked (eos masked: min_len covers the run)."""

    def __init__(self, lm, lens, seed=5):
        self.lm, self.K, self.enc = lm, lm.k, lm.llm
        gen = torch.Generator().manual_seed(seed)
        self.x = [self.K.put(torch.randn(n + 1, lm.llm_input_size, generator=gen)) for n in lens]
        self.lens = lens

    def prefill(self, j, cap=None):
        state = CK._KVState(self.K, self.enc.n_layers, self.enc.d, cap) if cap else None
        return self.enc.forward_chunk(self.x[j][:self.lens[j]], state)[1]

    def first(self, j):
        return self.x[j][self.lens[j]:self.lens[j] + 1].contiguous()

    def sp(self, max_len=64, min_len=64):
        return SamplingC(0, self.lm.eos_token, 1, min_len, max_len, 0.8, 25, 10, 0.1, 0, 0)

    def alone(self, j, tokens):
        """cv_lm1_step on sequence j alone, fed the tokens the batch emitted: per-step logits and the cache rows it leaves behind."""
        state, x, out = self.prefill(j), self.first(j), []
        for tok in tokens:
            logits = self.enc.fused_step(self.lm.step, x, state).cpu().clone()
            masked = logits.clone()
            masked[self.lm.eos_token] = -float("inf")
            assert int(masked.argmax()) == tok
            out.append(logits)
            x = self.lm.speech_emb[tok:tok + 1]
        return out, [r[:state.len].cpu().clone() for r in state.rows]


def _run_batch(seqs, nb, where, n_steps, small_cap=None):
    """Sequences `where` = {slot: sequence index} stepped one step per call on a batch of nb slots.  small_cap = (slot, cap): that slot's cache starts with `cap` rows and is
    grown and rebound while it runs.  Returns per slot (tokens, per-step logits, cache rows)."""
    lm, enc = seqs.lm, seqs.enc
    step = enc.make_step(lm.decoder, bf16=lm.w16)
    enc.batch_begin(step, nb)
    states, grew = {}, 0
    for slot, j in where.items():
        small = small_cap is not None and small_cap[0] == slot
        states[slot] = seqs.prefill(j, small_cap[1] if small else None)
        enc.batch_open(step, slot, seqs.first(j), states[slot], seqs.sp(), lm.speech_emb, reserve=not small)
    toks, logits = {s: [] for s in where}, {s: [] for s in where}
    for _ in range(n_steps):
        if small_cap is not None:
            st = states[small_cap[0]]
            if st.len + 1 > st.cap:
                st.reserve(st.len + 1)                              # new buffers: batch_steps rebinds the slot, its position and request are kept
                grew += 1
        out = enc.batch_steps(step, states, 1)
        for slot in where:
            assert out[slot][1] is False and len(out[slot][0]) == 1
            toks[slot] += out[slot][0]
            logits[slot].append(enc.batch_logits(step, slot, lm.decoder.n).clone())
    assert small_cap is None or grew >= 1
    rows = {s: [r[:states[s].len].cpu().clone() for r in states[s].rows] for s in where}
    for slot in where:
        enc.batch_release(step, slot)
    return toks, logits, rows


@pytest.mark.parametrize("size", ["tiny", "middle"])
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_batched_step_has_the_bits_of_the_single_step(lib, size, dtype):
    """Three sequences with prompts of 5, 3 and 1 rows on a batch of 3 slots, 10 steps: after every step each slot's logits equal cv_lm1_step on that sequence alone, at
    the end so do the cache rows of every layer - at the 128-wide test model and at d 512 / ffn 1280 (the whole-row form for N >= 2048 and the K-split form for K > 1024,
    the forms of the full model), over fp32 and bf16 matrices.  One slot's cache starts too small and is grown and rebound mid-run.  The same sequence in slot 0 of 1 and
    in slot 7 of 8 (the others empty) gives the same bits again."""
    lm = _lm(lib, CFG if size == "tiny" else MID, sampling="greedy", weight_dtype=dtype)
    seqs, n = _Seqs(lm, (5, 3, 1)), 10
    toks, logits, rows = _run_batch(seqs, 3, {0: 0, 1: 1, 2: 2}, n, small_cap=(1, 6))
    ref = {}
    for j in range(3):
        ref[j] = seqs.alone(j, toks[j])
        assert len(logits[j]) == n and all(torch.equal(a, b) for a, b in zip(logits[j], ref[j][0]))
        assert len(rows[j]) == lm.llm.n_layers and all(torch.equal(a, b) for a, b in zip(rows[j], ref[j][1]))
    assert len({tuple(v) for v in toks.values()}) == 3             # (three different sequences)
    for nb, slot in ((1, 0), (8, 7)):
        tk, lg, rw = _run_batch(seqs, nb, {slot: 0}, n)
        assert tk[slot] == toks[0] and all(torch.equal(a, b) for a, b in zip(lg[slot], ref[0][0])) and all(torch.equal(a, b) for a, b in zip(rw[slot], ref[0][1]))


@pytest.mark.parametrize("chunk", [3, 64])
def test_inference_batch_tokens(lib, chunk):
    """inference_batch on [zero-shot request, sft-shaped request]: the ids of the REAL class's golden, which are those of `inference` called sequentially; five requests of
    differing lengths and budgets on two slots (slots refill; eos and max_len arrive mid-chunk): every request equals its own sequential result."""
    g, kw, sft = _requests()
    lm = _lm(lib, sampling="greedy", decode_chunk=chunk)
    got = _collect(lm.inference_batch([kw, sft]), 2)
    assert got == [g["tokens_greedy"].tolist(), g["tokens_sft"].tolist()]
    assert got == [list(lm.inference(**kw)), list(lm.inference(**sft))]
    reqs = _five()
    want = [list(lm.inference(**r)) for r in reqs]
    assert _collect(lm.inference_batch(reqs, slots=2), 5) == want and len({len(w) for w in want}) >= 3
    assert lm.step_stat("batch_steps") > 0 and len(lm._loop_steps) == 1      # one handle, back in the pool
    assert _collect(lm.inference_batch(reqs[:3], slots=8, max_token_text_ratio=9), 3) == want[:3]      # (a request's own ratios win)
    host = _lm(lib, sampling=lambda scores, decoded, sampling: int(scores.argmax().item()))
    with pytest.raises(RuntimeError, match="device sampler"):
        next(host.inference_batch([kw]))
    with pytest.raises(ValueError, match="1..8 slots"):
        next(lm.inference_batch([kw], slots=9))


def test_inference_batch_ras(lib):
    """Repetition-aware sampling: with injected uniform variates (the 2 x 64 of the device-loop test) every request equals its sequential result; with the seeded device
    RNG the batch equals sequential calls on a fresh object with the same seed (request i draws from seed + i + 1 either way)."""
    _, kw, sft = _requests()
    reqs = [kw, sft] + _five()[:2]
    lm = _lm(lib, sampling="ras", decode_chunk=7)
    lm._uniforms = torch.rand(2 * 64, generator=torch.Generator().manual_seed(21))
    want = [list(lm.inference(**r)) for r in reqs]
    assert _collect(lm.inference_batch(reqs, slots=3), 4) == want and len(set(want[0])) > 3
    a, b = _lm(lib, sampling="ras", decode_chunk=7, seed=11), _lm(lib, sampling="ras", decode_chunk=7, seed=11)
    got = _collect(a.inference_batch(reqs, slots=4), 4)
    assert got == [list(b.inference(**r)) for r in reqs]
    assert got != want and a._request == b._request == 4


def test_slots_are_isolated(lib):
    """A request whose max_len ends it after 3 tokens shares the step with a long one and stays in the step as a `done` slot, a third slot is empty: the long one's logits
    and cache rows are those it has alone, the finished one's rows beyond its position are untouched (under the emulator every buffer ends at a guard page).  A batch
    generator closed early frees its slots and returns the handle; the next `inference` call is unaffected."""
    lm = _lm(lib, sampling="greedy", decode_chunk=2)
    seqs, enc, n = _Seqs(lm, (4, 2)), lm.llm, 8
    step = enc.make_step(lm.decoder)
    enc.batch_begin(step, 3)
    states = {0: seqs.prefill(0), 1: seqs.prefill(1)}
    enc.batch_open(step, 0, seqs.first(0), states[0], seqs.sp(), lm.speech_emb)
    enc.batch_open(step, 1, seqs.first(1), states[1], seqs.sp(max_len=3, min_len=3), lm.speech_emb)
    toks, logits, fin = {0: [], 1: []}, [], {}
    for _ in range(n):
        out = enc.batch_steps(step, states, 1)
        for s in (0, 1):
            toks[s] += out[s][0]
            fin[s] = out[s][1]
        logits.append(enc.batch_logits(step, 0, lm.decoder.n).clone())
    assert len(toks[0]) == n and len(toks[1]) == 3 and fin == {0: False, 1: True}
    ref_l, ref_r = seqs.alone(0, toks[0])
    assert all(torch.equal(a, b) for a, b in zip(logits, ref_l))
    assert all(torch.equal(r[:states[0].len].cpu(), b) for r, b in zip(states[0].rows, ref_r))
    _, short_r = seqs.alone(1, toks[1])
    assert states[1].len == 2 + 3
    for r, b in zip(states[1].rows, short_r):
        assert torch.equal(r[:5].cpu(), b) and float(r[6:].abs().max()) == 0.0      # (row 5 is the one a finished slot keeps rewriting)
    enc.batch_release(step, 0)
    enc.batch_release(step, 1)
    g, kw, sft = _requests()
    gen = lm.inference_batch([kw, sft], slots=2)
    i, first = next(gen)
    gen.close()
    assert first == g["tokens_greedy"].tolist()[:len(first)] and i == 0 and len(lm._loop_steps) == 1
    assert list(lm.inference(**kw)) == g["tokens_greedy"].tolist()
    assert _collect(lm.inference_batch([sft, kw], slots=2), 2) == [g["tokens_sft"].tolist(), g["tokens_greedy"].tolist()]


def _zero_handle(emu_lib, keep, n_out=10):
    from cosyvoice_amd._lib import ACT, Lm1Config, Lm1LayerWeights
    d, ffn = 64, 128

    def buf(*shape):
        keep.append(torch.zeros(*shape, dtype=torch.float32))
        return keep[-1].data_ptr()
    lw = (Lm1LayerWeights * 1)()
    for name, shape in (("ln1_g", (d,)), ("ln1_b", (d,)), ("w_qkv", (4 * d, d)), ("b_qkv", (4 * d,)), ("w_out", (d, d)), ("b_out", (d,)), ("ln2_g", (d,)), ("ln2_b", (d,)),
                        ("w1", (ffn, d)), ("b1", (ffn,)), ("w2", (d, ffn)), ("b2", (d,))):
        setattr(lw[0], name, buf(*shape))
    c = Lm1Config()
    c.n_layers, c.d, c.heads, c.ffn, c.d_in, c.n_out, c.act, c.xscale = 1, d, 1, ffn, d, n_out, ACT["relu"], 8.0
    for name, shape in (("embed_w", (d, d)), ("embed_b", (d,)), ("embed_g", (d,)), ("embed_beta", (d,)), ("after_g", (d,)), ("after_b", (d,)), ("dec_w", (n_out, d)), ("dec_b", (n_out,))):
        setattr(c, name, buf(*shape))
    h = C.c_void_p(emu_lib.raw("cv_lm1_create", C.c_void_p)(C.byref(c), lw))
    assert h
    return h, d


def test_batch_entry_points_check_their_arguments(emu_lib):
    """cv_lm1_batch_*: a slot count out of range, an unbound or unopened slot, a position or step count past a slot's cache, unaligned pointers and more logits than the
    sampler holds are errors with a message, not aborts; the header declares the entry points and both libraries export them."""
    from cosyvoice_amd._lib import CosyVoiceAmdError
    from cosyvoice_amd.build import build_hip
    from test_abi import declared_symbols
    names = ["cv_lm1_batch_" + n for n in ("begin", "bind", "open", "decode", "release", "logits")]
    hip = C.CDLL(build_hip())
    assert all(n in declared_symbols() and hasattr(hip, n) and hasattr(emu_lib.dll, n) for n in names)
    keep, i32 = [], C.c_int32
    big, _ = _zero_handle(emu_lib, keep, n_out=8200)
    h, d = _zero_handle(emu_lib, keep)
    try:
        with pytest.raises(CosyVoiceAmdError, match="at most 8192 logits"):
            emu_lib.cv_lm1_batch_begin(big, i32(2), None)
        rows, tabs, x, emb = torch.zeros(8, 4 * d), torch.zeros(2 * 8 - 1, d), torch.zeros(d + 4), torch.zeros(10, d)
        pr, pt = (C.c_void_p * 1)(rows.data_ptr()), (C.c_void_p * 1)(tabs.data_ptr())
        sp = SamplingC(0, 9, 1, 0, 4, 0.8, 25, 10, 0.1, 0, 0)
        xp, ep = C.c_void_p(x.data_ptr()), C.c_void_p(emb.data_ptr())
        toks, n_out, fin = (i32 * 16)(), (i32 * 2)(), (i32 * 2)()
        with pytest.raises(CosyVoiceAmdError, match="cv_lm1_batch_begin first"):
            emu_lib.cv_lm1_batch_bind(h, i32(0), pr, pt, i32(8), i32(8), None)
        for nb in (0, 9):
            with pytest.raises(CosyVoiceAmdError, match="1..8 slots"):
                emu_lib.cv_lm1_batch_begin(h, i32(nb), None)
        emu_lib.cv_lm1_batch_begin(h, i32(2), None)
        with pytest.raises(CosyVoiceAmdError, match="slot out of range"):
            emu_lib.cv_lm1_batch_bind(h, i32(2), pr, pt, i32(8), i32(8), None)
        with pytest.raises(CosyVoiceAmdError, match="n_tab >= cap"):
            emu_lib.cv_lm1_batch_bind(h, i32(0), pr, pt, i32(4), i32(8), None)
        with pytest.raises(CosyVoiceAmdError, match="16B aligned"):
            emu_lib.cv_lm1_batch_bind(h, i32(0), (C.c_void_p * 1)(rows.data_ptr() + 4), pt, i32(8), i32(8), None)
        with pytest.raises(CosyVoiceAmdError, match="cv_lm1_batch_bind first"):
            emu_lib.cv_lm1_batch_open(h, i32(0), xp, i32(0), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="no open slot"):
            emu_lib.cv_lm1_batch_decode(h, i32(1), toks, n_out, fin, None)
        emu_lib.cv_lm1_batch_bind(h, i32(0), pr, pt, i32(8), i32(8), None)
        with pytest.raises(CosyVoiceAmdError, match="no open slot"):                 # bound, not opened
            emu_lib.cv_lm1_batch_decode(h, i32(1), toks, n_out, fin, None)
        with pytest.raises(CosyVoiceAmdError, match="holds no request"):
            emu_lib.cv_lm1_batch_logits(h, i32(0), C.c_void_p(x.data_ptr()), None)
        with pytest.raises(CosyVoiceAmdError, match="beyond the bound cache"):
            emu_lib.cv_lm1_batch_open(h, i32(0), xp, i32(8), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="unaligned"):
            emu_lib.cv_lm1_batch_open(h, i32(0), C.c_void_p(x.data_ptr() + 4), i32(0), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="slot out of range"):
            emu_lib.cv_lm1_batch_open(h, i32(5), xp, i32(0), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="bad sampling parameters"):      # a token capacity below max_len
            emu_lib.cv_lm1_batch_open(h, i32(0), xp, i32(0), C.byref(sp), ep, i32(3), None, i32(0), None)
        emu_lib.cv_lm1_batch_open(h, i32(0), xp, i32(6), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="holds a request"):
            emu_lib.cv_lm1_batch_open(h, i32(0), xp, i32(0), C.byref(sp), ep, i32(4), None, i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="ends before these steps"):
            emu_lib.cv_lm1_batch_decode(h, i32(3), toks, n_out, fin, None)
        with pytest.raises(CosyVoiceAmdError, match="bad arguments"):
            emu_lib.cv_lm1_batch_decode(h, i32(0), toks, n_out, fin, None)
        emu_lib.cv_lm1_batch_decode(h, i32(2), toks, n_out, fin, None)               # zero weights: token 0 twice; the other slot is empty
        assert list(n_out) == [2, 0] and list(fin) == [0, 1] and toks[0] == toks[1] == 0
        with pytest.raises(CosyVoiceAmdError, match="slot out of range"):
            emu_lib.cv_lm1_batch_release(h, i32(2))
        emu_lib.cv_lm1_batch_release(h, i32(0))
        with pytest.raises(CosyVoiceAmdError, match="no open slot"):
            emu_lib.cv_lm1_batch_decode(h, i32(1), toks, n_out, fin, None)
        assert emu_lib.raw("cv_lm1_stat", C.c_int64)(h, b"batch_steps") == 2
    finally:
        emu_lib.raw("cv_lm1_destroy", None)(h)
        emu_lib.raw("cv_lm1_destroy", None)(big)


def test_tts_batch_matches_tts(lib):
    """CosyVoiceModel.tts_batch on two requests: for each the waveform of `tts` on it alone (the flow and the vocoder draw from torch's host RNG: reseeded identically
    before each request's token2wav in both runs), the per-uuid dicts empty afterwards."""
    g = gold("cv1k_llm")
    gen = torch.Generator().manual_seed(9)
    m = CK.CosyVoiceModel(_lm(lib, sampling="greedy", decode_chunk=5), build_flow(lib), build_hift(lib))
    reqs = [dict(text=g["text"][:, :4], llm_embedding=g["embedding"], flow_embedding=g["embedding"], max_token_text_ratio=3, min_token_text_ratio=3),
            dict(text=torch.randint(0, CFG.text_vocab, (1, 3), generator=gen, dtype=torch.int32), llm_embedding=torch.randn(1, CFG.spk_dim, generator=gen),
                 flow_embedding=torch.randn(1, CFG.spk_dim, generator=gen), max_token_text_ratio=4, min_token_text_ratio=4)]
    t2w = m.token2wav

    def seeded(**kw):
        torch.manual_seed(77)
        return t2w(**kw)
    m.token2wav = seeded
    inf = m.llm.inference
    alone = []
    for r in reqs:
        m.llm.inference = lambda _r=r, **kw: inf(**dict(kw, max_token_text_ratio=_r["max_token_text_ratio"], min_token_text_ratio=_r["min_token_text_ratio"]))
        alone.append(next(iter(m.tts(stream=False, **r)))["tts_speech"])
    m.llm.inference = inf
    got = dict(m.tts_batch(reqs, slots=2))
    assert sorted(got) == [0, 1]
    for i, want in enumerate(alone):
        assert want.shape == (1, int(reqs[i]["text"].shape[1] * reqs[i]["max_token_text_ratio"] / 50 * 22050 / 256) * 256) and float(want.abs().max()) > 0
        assert torch.equal(got[i]["tts_speech"], want)
    assert not (m.tts_speech_token_dict or m.llm_end_dict or m.mel_overlap_dict or m.flow_cache_dict or m.hift_cache_dict)
