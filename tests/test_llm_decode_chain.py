"""The batch-1 decode chain's `down` projection with its input staged once per workgroup in LDS (llm_kernels.h gemv_kernel<10, 1, 4, 0, true>), against the
form it replaces and against the oracle.

CV_DOWN_XLDS=0 at handle creation restores the form in which every 16-lane group fetches its own copy of the input.  The staged form feeds the same
values into the same FMAs in the same order, so logits are compared bit for bit.  The branch is taken from inter = 1024 (8 k-steps) up; the tiny model
of the other LM tests (inter = 256) never reaches it.

There is no read-back of the KV cache in the C API: the cache rows are covered through the logits of the later steps, which attend over them.

Second part: the decode attention (csrc/decode_attn.h, shared by the kernels of llm_kernels.h and llm_batch_kernels.h) walked across the exact edge of a wave pass."""
import ctypes as C
import dataclasses

import pytest
import torch

from cosyvoice_amd.llm import Qwen2LM
from cosyvoice_amd import synthetic as W
from oracle import llm as OL

N_STEPS = 12
# 8 k-steps: the smallest K of the branch, two per wave | 9: split 2 / 2 / 2 / 3, the zero-filled slots of the shorter waves | 40: the bound gemv() checks, all of the LDS image
INTERS = [1024, 1152, 5120]


@pytest.fixture(scope="module")
def models():
    """(cfg, state dict, utterance, oracle tokens, oracle log-probabilities) per `inter`, computed once."""
    out = {}
    for inter in INTERS:
        cfg = dataclasses.replace(W.tiny()[0], inter=inter)
        assert cfg.hidden == 128
        sd = W.make_llm(cfg)
        u = W.synthetic_utterance(cfg, W.tiny()[1], n_prompt_tok=11, n_prompt_text=5, n_text=6, seed=7)
        trace = {}
        want = OL.inference(sd, cfg, u["text"], u["prompt_text"], u["llm_prompt_speech_token"], max_token_text_ratio=2, min_token_text_ratio=2, trace=trace)
        assert len(want) == N_STEPS
        out[inter] = (cfg, sd, u, want, trace["logp"])
    return out


def _kw(u):
    t = lambda n: torch.tensor([n], dtype=torch.int32)
    return dict(text=u["text"], text_len=t(u["text"].shape[1]), prompt_text=u["prompt_text"], prompt_text_len=t(u["prompt_text"].shape[1]),
                prompt_speech_token=u["llm_prompt_speech_token"], prompt_speech_token_len=t(u["llm_prompt_speech_token"].shape[1]),
                embedding=u["llm_embedding"])


def _lm(monkeypatch, lib, sd, cfg, xlds, **kw):
    monkeypatch.setenv("CV_DOWN_XLDS", "1" if xlds else "0")           # read when the handle is created
    return Qwen2LM(sd, cfg, lib=lib, max_len=128, sampling="greedy", **kw)


def _step_logits(lm, u, n):
    lm.prefill(lm.build_lm_input(u["text"], u["prompt_text"], u["llm_prompt_speech_token"]))
    sp = lm.make_sampling(n, n)
    toks, logits = [], []
    for _ in range(n):
        t, _fin = lm.decode(1, sp)
        toks += t
        logits.append(lm.last_logits().clone())
    return toks, logits


@pytest.mark.parametrize("inter", INTERS)
def test_down_xlds_has_the_bits_of_the_per_group_fetch(lib, models, monkeypatch, inter):
    cfg, sd, u, want, logp = models[inter]
    toks0, log0 = _step_logits(_lm(monkeypatch, lib, sd, cfg, False), u, N_STEPS)
    toks1, log1 = _step_logits(_lm(monkeypatch, lib, sd, cfg, True), u, N_STEPS)
    assert toks0 == want and toks1 == want
    for i in range(N_STEPS):
        assert torch.equal(log0[i], log1[i]), (inter, i, (log0[i] - log1[i]).abs().max().item())
        torch.testing.assert_close(log1[i].log_softmax(-1), logp[i], rtol=1e-4, atol=1e-4)      # (and both are right)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("inter", INTERS)
def test_down_xlds_greedy_tokens(lib, models, monkeypatch, inter, use_graph):
    cfg, sd, u, want, _ = models[inter]
    lm = _lm(monkeypatch, lib, sd, cfg, True, decode_chunk=5, use_graph=use_graph)
    assert list(lm.inference(**_kw(u), max_token_text_ratio=2, min_token_text_ratio=2)) == want


# ---- the decode attention at the edge of a pass.  A wave of attn_decode_kernel takes 48 keys per pass (12 slots x 4 lane groups), a workgroup of the batched VALU
# form 4 x 48 = 192, the MFMA form 16-key tiles.  Three decode steps from a context of 48 * slices - 1: the new token sits at index 48 * slices - 1 (every slice one
# full pass), then 48 * slices and 48 * slices + 1 (slices of 52 keys: a full pass and a second one that holds 1 - 4 keys; the last slice is short).
PASS = 48
EDGE_STEPS = 3


@pytest.fixture(scope="module")
def edge():
    """(cfg, state dict, {start context: [(request, oracle tokens, oracle log-probabilities), ..]}): three requests at 191 (the batch; the first also alone), one at 383."""
    cfg = W.tiny()[0]
    sd = W.make_llm(cfg)
    out = {}
    for start, seeds in ((4 * PASS - 1, (34, 35, 36)), (8 * PASS - 1, (35,))):       # (seeds whose oracle run does not stop on a special id within the walk)
        out[start] = []
        for seed in seeds:
            u = W.synthetic_utterance(cfg, W.tiny()[1], n_prompt_tok=start - 7, n_prompt_text=2, n_text=EDGE_STEPS, seed=seed)     # rows: sos + 2 + 3 + task id + prompt tokens
            trace = {}
            want = OL.inference(sd, cfg, u["text"], u["prompt_text"], u["llm_prompt_speech_token"], max_token_text_ratio=2, min_token_text_ratio=1, trace=trace)
            assert len(want) >= EDGE_STEPS
            out[start].append((u, want, trace["logp"]))
    return cfg, sd, out


@pytest.mark.parametrize("splits", [4, 8])
def test_attention_pass_boundary_single_sequence(lib, edge, splits):
    cfg, sd, reqs = edge
    start = splits * PASS - 1
    u, want, logp = reqs[start][0]
    lm = Qwen2LM(sd, cfg, lib=lib, max_len=512, sampling="greedy", attn_splits=splits)
    x = lm.build_lm_input(u["text"], u["prompt_text"], u["llm_prompt_speech_token"])
    assert x.shape[0] == start
    lm.prefill(x)
    sp = lm.make_sampling(EDGE_STEPS, 2 * EDGE_STEPS)
    for i in range(EDGE_STEPS):                                        # the new token at index start + i
        toks, _fin = lm.decode(1, sp)
        assert toks == [want[i]], (splits, i)
        torch.testing.assert_close(lm.last_logits().log_softmax(-1), logp[i], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("form", [0, 1])
def test_attention_pass_boundary_batch(lib, edge, form):
    """Three lock-step slots at 191 -> 193, the per-head VALU form (0) and the MFMA form (1) pinned."""
    cfg, sd, reqs = edge
    start, nb = 4 * PASS - 1, 3
    lm = Qwen2LM(sd, cfg, lib=lib, max_len=256, sampling="greedy", decode_chunk=1)
    lib.cv_llm_set_option(lm._h, b"batch_attn", C.c_int32(form))
    st = None
    lib.cv_llm_batch_begin(lm._h, C.c_int32(nb), st)
    inputs = [lm.build_lm_input(u["text"], u["prompt_text"], u["llm_prompt_speech_token"]) for u, _, _ in reqs[start]]
    assert [x.shape[0] for x in inputs] == [start] * nb
    lm._prefill_slots(list(range(nb)), inputs, [lm.make_sampling(EDGE_STEPS, 2 * EDGE_STEPS) for _ in range(nb)], st)
    logits = torch.empty(cfg.speech_token_size + cfg.n_special, dtype=torch.float32)
    for i in range(EDGE_STEPS):
        buf, n_out, f = (C.c_int32 * nb)(), (C.c_int32 * nb)(), (C.c_int32 * nb)()
        lib.cv_llm_batch_decode(lm._h, C.c_int32(1), buf, n_out, f, st)
        for b, (_, want, logp) in enumerate(reqs[start]):
            assert n_out[b] == 1 and buf[b] == want[i], (form, i, b)
            lib.cv_llm_batch_logits(lm._h, C.c_int32(b), C.c_void_p(logits.data_ptr()), st)
            torch.testing.assert_close(logits.log_softmax(-1), logp[i], rtol=1e-4, atol=1e-4)
