"""The batch-1 decode chain's `down` projection with its input staged once per workgroup in LDS (llm_kernels.h gemv_kernel<10, 1, 4, 0, true>), against the
form it replaces and against the oracle.

CV_DOWN_XLDS=0 at handle creation restores the form in which every 16-lane group fetches its own copy of the input.  The staged form feeds the same
values into the same FMAs in the same order, so logits are compared bit for bit.  The branch is taken from inter = 1024 (8 k-steps) up; the tiny model
of the other LM tests (inter = 256) never reaches it.

There is no read-back of the KV cache in the C API: the cache rows are covered through the logits of the later steps, which attend over them."""
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
