"""The integer options of the flow and LM handles (csrc/options.h, the tables kFlowOptions / kLlmOptions): what each option accepts, by name and through its
environment variable.  The lists below are this file's own statement of the contract - they are not read from the library - and the completeness test holds them
against the C sources: an option added to a table without a line here fails."""
import ctypes as C
import os
import re

import pytest
import torch

from cosyvoice_amd._lib import CosyVoiceAmdError
from cosyvoice_amd.flow import CausalMaskedDiffWithXvec
from cosyvoice_amd.llm import Qwen2LM
from cosyvoice_amd import synthetic as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cosyvoice_amd", "csrc")
BIG = 2 ** 31 - 1


def O(name, legal, illegal=None, gated=()):
    """legal: values that return 0; illegal: one value the option refuses (None: it has no check); gated: the legal values that need a CV_BUILD_EXPERIMENTS library"""
    return dict(name=name, legal=tuple(legal), illegal=illegal, gated=tuple(gated))


BOOL = (0, 1, 7, -1)
FLOW_OPTIONS = [
    O("use_graph", BOOL), O("bf16_mfma", BOOL), O("fused", BOOL),
    O("flow_tile", range(0, 5), 5), O("flow_ntile", (0, 1, 2), 3), O("res_tile", (0, 1), 2),
    O("attn32", BOOL, gated=(0,)), O("attn32_waves", (0, 2, 4), 3),
    O("attn_waves", (2, 4), 3), O("attn_kt", (1, 2), 0), O("attn_ks", (1, 2, 3, 4), 5),
    O("attn2_rows", (0, 1, 4000, BIG), -1), O("big_rows", (0, 1, 2000, BIG), -1),
    O("big_tile0", range(0, 5), 7), O("big_tile1", range(0, 5), -1), O("big_persist", range(-1, 9), 99), O("big_grid_cap", (0, 3, BIG), -1),
    O("big_glds", BOOL), O("big_lds_epi", BOOL),
    O("fused_band", BOOL), O("band_qkv", BOOL), O("ln_qkv", BOOL),
    O("band_bm", (0, 32, 48, 64), 17), O("band_pipe", (0, 1, 2), 9), O("band_stagger", (0, 1, 64), 65, gated=(1, 64)),
    O("fused_tail", BOOL, gated=(1, 7, -1)), O("tail_ring", (8, 16, 0, 99, -5)),
    O("est_streams", (1, 2), 3), O("eager_streams", (1, 2), 0, gated=(2,)), O("enc_batch", BOOL),
    O("graph_max_rows", (0, 1, 1000, BIG), -1), O("graph_cap", (1, 32, 256), 0),
    O("gemm_dbg", (0, 1, 4, 0)), O("attn_dbg", (0, 1, 0)),
]
LLM_OPTIONS = [
    O("use_graph", BOOL), O("head_rows", (1, 2), 3), O("head_waves", (4, 7), 5), O("attn_splits", (4, 8, 16), 6),
    O("fused_qkv_attn", BOOL, gated=(1, 7, -1)), O("prefetch", (0, 1, 2), 3, gated=(1, 2)), O("prefetch_shift", (0, 1, -3, 100)),
    O("fused_attn_oproj", (0, 1, 2), gated=(1, 2)), O("oproj_rblocks", (4, 8), 6), O("oproj_waves", (8, 16), 4),
    O("prefill_rows", BOOL), O("batch_attn", (-1, 0, 1, 2), 3), O("batch_packed", BOOL),
    O("batch_fp8", (0,), 1),                 # (the tiny model registers no fp8 tensors: 1 is refused)
]
# the state the rest of a session expects of a handle that is still alive (the module-scoped ones below): the defaults
FLOW_DEFAULTS = dict(use_graph=1, bf16_mfma=0, fused=1, flow_tile=0, flow_ntile=0, res_tile=1, attn32=1, attn32_waves=0, attn_waves=4, attn_kt=1, attn_ks=2, attn2_rows=0, big_rows=2000,
                     big_tile0=0, big_tile1=0, big_persist=-1, big_grid_cap=0, big_glds=0, big_lds_epi=1, fused_band=1, band_qkv=1, ln_qkv=1, band_bm=0, band_pipe=2, band_stagger=0,
                     fused_tail=0, tail_ring=8, est_streams=1, eager_streams=1, enc_batch=1, graph_max_rows=1000, graph_cap=32, gemm_dbg=0, attn_dbg=0)


@pytest.fixture(scope="module")
def tiny():
    cfg = W.tiny()[1]
    return cfg, W.make_flow(cfg)


def _check_options(lib, setter, handle, options, what):
    for o in options:
        name = o["name"].encode()
        for v in o["legal"]:
            if v in o["gated"] and not lib.experiments:
                with pytest.raises(CosyVoiceAmdError, match="built without") as e:
                    setter(handle, name, C.c_int32(v))
                assert o["name"] in str(e.value), (what, o["name"], v, str(e.value))
            else:
                setter(handle, name, C.c_int32(v))                      # raises on a non-zero return
        if o["illegal"] is not None:
            with pytest.raises(CosyVoiceAmdError) as e:
                setter(handle, name, C.c_int32(o["illegal"]))
            assert o["name"] in str(e.value) and "unknown option" not in str(e.value), (what, o["name"], str(e.value))
    for bad in (b"nope", b"", b"flow_tile ", b"CV_FLOW_BAND_BM"):
        with pytest.raises(CosyVoiceAmdError, match="unknown option"):
            setter(handle, bad, C.c_int32(1))


def test_flow_options_accept_and_refuse(lib, tiny):
    cfg, sd = tiny
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    _check_options(lib, lib.cv_flow_set_option, flow._h, FLOW_OPTIONS, "flow")
    assert set(FLOW_DEFAULTS) == {o["name"] for o in FLOW_OPTIONS}
    for k, v in FLOW_DEFAULTS.items():                                   # every default is a legal value in every build
        lib.cv_flow_set_option(flow._h, k.encode(), C.c_int32(v))


def test_llm_options_accept_and_refuse(lib):
    cfg = W.tiny()[0]
    lm = Qwen2LM(W.make_llm(cfg), cfg, lib=lib, max_len=64, sampling="greedy")
    _check_options(lib, lib.cv_llm_set_option, lm._h, LLM_OPTIONS, "llm")


def _names_in_source(path, table, setter):
    """The rows of the option table `table` plus the names `setter` compares by hand (its special cases)."""
    src = open(os.path.join(CSRC, path)).read()
    body = src[src.index(table + "[] = {"):]
    rows = re.findall(r'^\s*\{"(\w+)",', body[:body.index("\n};")], re.M)
    fn = src[src.index("int " + setter + "("):]
    special = re.findall(r'std::string\(name\) == "(\w+)"', fn[:fn.index("\n}\n")])
    assert rows and len(set(rows)) == len(rows) and not set(rows) & set(special), (rows, special)
    return rows, special


@pytest.mark.parametrize("path,table,setter,options,n_special", [("flow.hip", "kFlowOptions", "cv_flow_set_option", FLOW_OPTIONS, 3),
                                                                 ("llm.hip", "kLlmOptions", "cv_llm_set_option", LLM_OPTIONS, 3)])
def test_the_lists_above_are_complete(path, table, setter, options, n_special):
    rows, special = _names_in_source(path, table, setter)
    listed = [o["name"] for o in options]
    assert len(set(listed)) == len(listed)
    assert set(rows) | set(special) == set(listed), sorted(set(rows) | set(special) ^ set(listed))
    assert len(special) == n_special, special                            # no chain of name comparisons grows back next to the table


def _estimate(flow, T=45, seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 80, T, generator=g); mu = torch.randn(2, 80, T, generator=g); cond = torch.randn(2, 80, T, generator=g)
    spk = torch.randn(2, 80, generator=g); t = torch.tensor([0.3, 0.3]); mask = torch.ones(2, 1, T)
    return flow.decoder.estimator(x, mask, mu, t, spk, cond, streaming=False).cpu().clone()


def _infer(flow, cfg, n=13):
    g = torch.Generator().manual_seed(5)
    t = lambda k: torch.tensor([k], dtype=torch.int32)
    return flow.inference(token=torch.randint(0, cfg.vocab, (1, n), generator=g, dtype=torch.int32), token_len=t(n),
                          prompt_token=torch.randint(0, cfg.vocab, (1, 7), generator=g, dtype=torch.int32), prompt_token_len=t(7),
                          prompt_feat=torch.randn(1, 14, 80, generator=g) * 2 - 5, prompt_feat_len=t(14), embedding=torch.randn(1, cfg.spk_dim, generator=g),
                          streaming=False, finalize=True)[0].cpu().clone()


def _stat(lib, flow, name):
    v = C.c_int64(0)
    lib.cv_flow_get_stat(flow._h, name, C.byref(v))
    return v.value


def test_environment_goes_through_the_option_checks(lib, tiny, monkeypatch):
    """cv_flow_finalize applies the variables of the table in-process, through the checks of the options."""
    cfg, sd = tiny
    cfg = __import__("dataclasses").replace(cfg, n_timesteps=2)
    # a legal value is taken: with CV_FLOW_GRAPH_MAX_ROWS=1 no solve is ever captured (the default captures this shape on its second sighting) ...
    monkeypatch.setenv("CV_FLOW_GRAPH_MAX_ROWS", "1")
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    a, b = _infer(flow, cfg), _infer(flow, cfg)
    assert torch.equal(a, b) and _stat(lib, flow, b"graph_captures") == 0
    monkeypatch.delenv("CV_FLOW_GRAPH_MAX_ROWS")
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    assert torch.equal(_infer(flow, cfg), a) and torch.equal(_infer(flow, cfg), a) and _stat(lib, flow, b"graph_captures") == 1
    # ... and it overrides what was set before finalize, as it always did
    monkeypatch.setenv("CV_FLOW_GRAPH_MAX_ROWS", "1")
    finalize = lib.cv_flow_finalize

    def set_then_finalize(h):
        lib.cv_flow_set_option(h, b"graph_max_rows", C.c_int32(0))
        finalize(h)
    monkeypatch.setattr(lib, "cv_flow_finalize", set_then_finalize, raising=False)
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    monkeypatch.undo()
    _infer(flow, cfg), _infer(flow, cfg)
    assert _stat(lib, flow, b"graph_captures") == 0
    # CV_FLOW_BAND_BM=32 is accepted and a large pass under it computes the bits of every other band height (what tests/test_flow_big.py holds the band shapes to)
    base = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, precision="bf16")
    lib.cv_flow_set_option(base._h, b"big_rows", C.c_int32(0))
    monkeypatch.setenv("CV_FLOW_BAND_BM", "32"); monkeypatch.setenv("CV_FLOW_BIG_ROWS", "1")
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, precision="bf16")
    assert any(k.endswith(".band") for k in flow._tensors)
    assert torch.equal(_estimate(flow), _estimate(base))
    monkeypatch.delenv("CV_FLOW_BIG_ROWS")
    # a value the option refuses, or no integer at all, fails finalize under the variable's name
    for var, val, option in (("CV_FLOW_BAND_BM", "17", "band_bm"), ("CV_FLOW_BAND_PIPE", "x", "band_pipe"), ("CV_FLOW_BAND_PIPE", "9", "band_pipe"), ("CV_FLOW_BAND_PIPE", "1x", "band_pipe"),
                             ("CV_FLOW_BAND_PIPE", "", "band_pipe"), ("CV_FLOW_BIG_TILE0", "7", "big_tile0"), ("CV_FLOW_BIG_PERSIST", "99", "big_persist"), ("CV_FLOW_RES_TILE", "2", "res_tile"),
                             ("CV_FLOW_ATTN32_WAVES", "3", "attn32_waves"), ("CV_FLOW_EAGER_STREAMS", "3", "eager_streams")):
        monkeypatch.delenv("CV_FLOW_BAND_BM", raising=False)
        monkeypatch.setenv(var, val)
        with pytest.raises(CosyVoiceAmdError, match=var) as e:
            CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
        assert option in str(e.value)
        monkeypatch.delenv(var)
    # a variable that selects an experiment fails finalize in a library built without them, and is taken in one built with them
    monkeypatch.setenv("CV_FLOW_EAGER_STREAMS", "2")
    if lib.experiments:
        CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    else:
        with pytest.raises(CosyVoiceAmdError, match="built without") as e:
            CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
        assert "CV_FLOW_EAGER_STREAMS" in str(e.value)


def test_llm_environment_goes_through_the_option_checks(lib, monkeypatch):
    cfg = W.tiny()[0]
    sd = W.make_llm(cfg)
    monkeypatch.setenv("CV_HEAD_WAVES", "7"); monkeypatch.setenv("CV_OPROJ_RBLOCKS", "8")
    Qwen2LM(sd, cfg, lib=lib, max_len=64, sampling="greedy")
    monkeypatch.setenv("CV_HEAD_WAVES", "5")
    with pytest.raises(CosyVoiceAmdError, match="CV_HEAD_WAVES") as e:
        Qwen2LM(sd, cfg, lib=lib, max_len=64, sampling="greedy")
    assert "head_waves" in str(e.value)
    monkeypatch.setenv("CV_HEAD_WAVES", "4"); monkeypatch.setenv("CV_DECODE_PREFETCH", "1")
    if lib.experiments:
        Qwen2LM(sd, cfg, lib=lib, max_len=64, sampling="greedy")
    else:
        with pytest.raises(CosyVoiceAmdError, match="built without"):
            Qwen2LM(sd, cfg, lib=lib, max_len=64, sampling="greedy")


def test_options_drop_the_captured_solves(lib, tiny):
    """An option that a captured Euler solve bakes in drops the graph cache when it is set; enc_batch and eager_streams, which no captured solve reads, keep it
    (the capture arrangement of tests/test_flow.py::test_graph_cache_evicts_least_recently_used)."""
    cfg, sd = tiny
    cfg = __import__("dataclasses").replace(cfg, n_timesteps=2)
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib)
    first = _infer(flow, cfg)                                            # the workspaces reach their final size before anything is captured
    for name, value, drops in (("flow_tile", 0, True), ("enc_batch", 0, False), ("eager_streams", 1, False), ("graph_cap", 8, True), ("tail_ring", 16, True),
                               ("band_bm", 48, True), ("use_graph", 1, True)):
        while _stat(lib, flow, b"graphs_cached") == 0:                   # captured on the second sighting
            assert torch.equal(_infer(flow, cfg), first)
        lib.cv_flow_set_option(flow._h, name.encode(), C.c_int32(value))
        assert _stat(lib, flow, b"graphs_cached") == (0 if drops else 1), name
        assert torch.equal(_infer(flow, cfg), first)
