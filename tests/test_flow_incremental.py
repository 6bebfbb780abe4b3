"""Incremental streaming flow (cv_flow_stream_open / _chunk / _close, CausalMaskedDiffWithXvec.open_stream): a stream returns, call by call, the frames that
`flow.inference(streaming=True, finalize=False)` on the same tokens returns, while solving only the NEW chunks - the earlier chunks' transformer K / V rows and
convolution halos are kept per Euler step and guidance row.  The yardsticks are the existing pass and the oracle, never the new path itself."""
import ctypes as C
import dataclasses

import pytest
import torch

from cosyvoice_amd import synthetic as W
from cosyvoice_amd._lib import CosyVoiceAmdError
from cosyvoice_amd.flow import CausalMaskedDiffWithDiT, CausalMaskedDiffWithXvec
from oracle import flow as OF

N_P = 5                                         # prompt tokens (10 prompt frames = one 10-frame chunk)
# token counts (prompt included) per call; 2 * (n_tok - 3) frames: 20, 30, 50, 60 (new chunks 1 + 1, 1, 2, 1) / 70, 130, 140 (key counts across the 64- and 128-key tile edges)
SCHEDULES = {"short": (13, 18, 28, 33), "long": (38, 68, 73)}
BF16_MARGIN = 1.10 * 1.5                        # worst measured ratio x safety factor: see test_bf16_chunks_stay_at_the_existing_pass_noise


@pytest.fixture(scope="module")
def tiny():
    cfg = dataclasses.replace(W.tiny()[1], chunk=5)
    return cfg, W.make_flow(cfg)


def _utt(cfg, n_total):
    g = torch.Generator().manual_seed(31)
    return dict(prompt_token=torch.randint(0, cfg.vocab, (1, N_P), generator=g, dtype=torch.int32),
                token=torch.randint(0, cfg.vocab, (1, n_total - N_P), generator=g, dtype=torch.int32),
                prompt_feat=torch.randn(1, 2 * N_P, 80, generator=g) * 2 - 5, embedding=torch.randn(1, cfg.spk_dim, generator=g))


_oracle = {}


def _oracle_mel(tiny, name, n_tok):
    """fp32 oracle of the existing pass at one call of a schedule: computed once, shared by the fp32 and bf16 tests and both backends, never modified."""
    cfg, sd = tiny
    if (name, n_tok) not in _oracle:
        u = _utt(cfg, SCHEDULES[name][-1])
        _oracle[(name, n_tok)] = OF.inference(sd, cfg, u["token"][:, :n_tok - N_P], u["prompt_token"], u["prompt_feat"], u["embedding"], streaming=True, finalize=False, n_timesteps=2)
    return _oracle[(name, n_tok)]


def _full(flow, u, n_tok):
    t = lambda n: torch.tensor([n], dtype=torch.int32)
    mel, _ = flow.inference(token=u["token"][:, :n_tok - N_P], token_len=t(n_tok - N_P), prompt_token=u["prompt_token"], prompt_token_len=t(N_P), prompt_feat=u["prompt_feat"],
                            prompt_feat_len=t(2 * N_P), embedding=u["embedding"], streaming=True, finalize=False)
    return mel.cpu()


def _run_stream(flow, u, schedule):
    outs = []
    with flow.open_stream(max_frames=400) as st:
        for n_tok in schedule:
            outs.append(st.chunk(u["token"][:, :n_tok - N_P], u["prompt_token"], u["prompt_feat"], u["embedding"]).cpu())
    return outs


@pytest.mark.parametrize("name,slices", [("short", 0), ("long", 0), ("long", 3)])
def test_chunks_equal_the_existing_pass(lib, tiny, name, slices):
    """fp32: every chunk against the existing pass on the same tokens, sliced to the same frames, at test_streaming_prefix_invariance's 1e-4 (two routes to the same
    chunk-causal frames), and against the oracle at test_inference's 1e-3.  slices = 3 on the long schedule: 70 / 130 / 140 keys are 2 / 3 / 3 tiles over three key
    slices - a slice of one tile, and at 70 keys an EMPTY third slice."""
    cfg, sd = tiny
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, n_timesteps=2)
    flow.lib.cv_flow_stream_slices(flow._h, C.c_int32(slices))
    u = _utt(cfg, SCHEDULES[name][-1])
    done = 2 * N_P
    for n_tok, got in zip(SCHEDULES[name], _run_stream(flow, u, SCHEDULES[name])):
        T1 = 2 * (n_tok - cfg.pre_lookahead)
        assert got.shape == (1, 80, T1 - done), (n_tok, got.shape)
        want = _full(flow, u, n_tok)[:, :, done - 2 * N_P:]
        print("fp32 %s n_tok %d: max |inc - full| = %.3e" % (name, n_tok, float((got - want).abs().max())))
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(got, _oracle_mel(tiny, name, n_tok)[:, :, done - 2 * N_P:], rtol=1e-3, atol=1e-3)
        done = T1


def test_bf16_chunks_stay_at_the_existing_pass_noise(lib, tiny):
    """bf16 mode, both schedules.  Statistic: max |mel - fp32 oracle mel| over the frames a call returns, for the incremental path and for the existing pass.  The
    attention of the incremental path sums a query's keys in another order (16-wide MFMA tiles and key slices against 32-wide tiles), which can flip the bf16 rounding
    of a probability either way, so its error may exceed the existing pass's.  Measured ratio inc / existing over the seven calls of this file: 1.000 .. 1.095 on the
    MI355X (errors 1.9e-2 .. 2.6e-2 both ways) and 0.824 .. 1.064 under the emulator; the margin is the worst ratio, 1.10, times a safety factor of 1.5: 1.65."""
    cfg, sd = tiny
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, n_timesteps=2, precision="bf16")
    for name, schedule in SCHEDULES.items():
        u = _utt(cfg, schedule[-1])
        done = 2 * N_P
        for n_tok, got in zip(schedule, _run_stream(flow, u, schedule)):
            ref = _oracle_mel(tiny, name, n_tok)[:, :, done - 2 * N_P:]
            e_inc = float((got - ref).abs().max())
            e_full = float((_full(flow, u, n_tok)[:, :, done - 2 * N_P:] - ref).abs().max())
            print("bf16 %s n_tok %d: max |inc - oracle| = %.4e, max |full - oracle| = %.4e, ratio %.3f" % (name, n_tok, e_inc, e_full, e_inc / e_full))
            assert got.shape == ref.shape and e_full > 1e-4                   # ... and the mode is really on
            assert e_inc <= BF16_MARGIN * e_full, (name, n_tok, e_inc, e_full)
            done = 2 * (n_tok - cfg.pre_lookahead)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_streams_on_one_handle_do_not_see_each_other(lib, tiny, precision):
    """Two requests interleaved call by call on ONE handle each equal their own solo run bit for bit; closing returns the cache bytes."""
    cfg, sd = tiny
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, n_timesteps=2, precision=precision)
    ua, ub = _utt(cfg, 33), _utt(cfg, 33)
    ub["token"] = (ub["token"] + 7) % cfg.vocab
    ub["embedding"] = ub["embedding"].flip(1)
    sched_a, sched_b = (13, 18, 33), (18, 23, 33)
    solo_a, solo_b = _run_stream(flow, ua, sched_a), _run_stream(flow, ub, sched_b)
    assert not torch.equal(solo_a[-1], solo_b[-1])
    bytes0 = flow.stat("stream_cache_bytes")
    assert bytes0 == 0 and flow.stat("open_streams") == 0
    sa, sb = flow.open_stream(max_frames=200), flow.open_stream(max_frames=200)
    for i in range(3):
        a = sa.chunk(ua["token"][:, :sched_a[i] - N_P], ua["prompt_token"], ua["prompt_feat"], ua["embedding"]).cpu()
        b = sb.chunk(ub["token"][:, :sched_b[i] - N_P], ub["prompt_token"], ub["prompt_feat"], ub["embedding"]).cpu()
        assert torch.equal(a, solo_a[i]) and torch.equal(b, solo_b[i]), (precision, i)
    inner, blocks = cfg.est_heads * 64, (cfg.est_mid + 2) * cfg.est_blocks
    assert flow.stat("stream_cache_bytes") >= 2 * 60 * 2 * inner * (2 if precision == "bf16" else 4) * blocks * 2 * 2      # two streams x 60 frames x (K, V) x blocks x steps x rows
    sa.close()
    assert 0 < flow.stat("stream_cache_bytes") and flow.stat("open_streams") == 1
    sb.close()
    sb.close()                                                                    # closing twice is harmless
    assert flow.stat("stream_cache_bytes") == bytes0 and flow.stat("open_streams") == 0
    with pytest.raises(ValueError, match="closed"):
        sb.chunk(ub["token"], ub["prompt_token"], ub["prompt_feat"], ub["embedding"])


def test_refused_calls_name_the_entry_point_and_leave_the_stream_usable(lib, tiny):
    cfg, sd = tiny
    flow = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, n_timesteps=2)
    u = _utt(cfg, 33)
    call = lambda st, n_tok, **kw: st.chunk(u["token"][:, :n_tok - N_P], u["prompt_token"], kw.get("prompt_feat", u["prompt_feat"]), u["embedding"]).cpu()
    want = _run_stream(flow, u, (13, 18))
    with flow.open_stream(max_frames=30) as st:
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: misaligned frame count"):
            call(st, 14)                                                          # 22 frames: not a multiple of 10
        assert torch.equal(call(st, 13), want[0])
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: no new chunk"):
            call(st, 13)
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: mel_len1 changed"):
            call(st, 18, prompt_feat=u["prompt_feat"][:, :8])
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: n_timesteps changed"):
            flow.n_timesteps = 3
            try:
                call(st, 18)
            finally:
                flow.n_timesteps = 2
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: 40 frames pass the stream's max_frames = 30"):
            call(st, 23)
        assert torch.equal(call(st, 18), want[1])                                 # the refused calls left the state alone
        other = CausalMaskedDiffWithXvec(sd, cfg, lib=lib, n_timesteps=2)
        got = C.c_int32(0)
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_chunk: the stream was opened on another handle"):
            lib.cv_flow_stream_chunk(other._h, st._s, C.c_void_p(1), C.c_int32(23), None, C.c_int32(10), C.c_void_p(1), C.c_void_p(1), C.c_int32(2), C.c_void_p(1), C.byref(got), None)
    with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_open: max_frames must hold at least one chunk"):
        flow.open_stream(max_frames=9)


def test_other_estimators_are_refused(lib):
    from cosyvoice_amd import cosyvoice1_hip as CK
    from cv1k_common import CFG
    cfg = W.tiny_cv3_flow()
    dit = CausalMaskedDiffWithDiT(W.make_flow_dit(cfg), cfg, lib=lib)
    with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_open: .*cfg.estimator == 0"):
        dit.open_stream()
    hd = CK.EstimatorHandle(W.make_cv1_flow(CFG), "decoder.estimator.", CFG.est_heads, lib, "fp32")
    s = C.c_void_p()
    with pytest.raises(CosyVoiceAmdError, match="cv_flow_stream_open: .*cfg.estimator == 0"):
        lib.cv_flow_stream_open(hd._h, C.c_int32(100), C.byref(s))
