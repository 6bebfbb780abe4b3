"""CosyVoice2Model.flow_incremental: the streaming chunks of tts(stream=True) through one incremental flow stream per request (flow.open_stream), the final call
through the existing pass.  Same fixture, oracle and tolerance as tests/test_model.py::test_tts_matches_oracle."""
import pytest
import torch

from oracle import llm as OL
from oracle import model as OM
from test_model import _build, setup  # noqa: F401  (the module-scoped fixture and the model builder of the streamed-request test)


def _tts(m, u):
    return [o["tts_speech"] for o in m.tts(text=u["text"], flow_embedding=u["flow_embedding"], llm_embedding=u["llm_embedding"], prompt_text=u["prompt_text"],
                                           llm_prompt_speech_token=u["llm_prompt_speech_token"], flow_prompt_speech_token=u["flow_prompt_speech_token"],
                                           prompt_speech_feat=u["prompt_speech_feat"], stream=True)]


def test_streamed_request_on_the_incremental_flow(lib, setup):
    cfgs, sds, u = setup
    lc, fc, hc = cfgs
    m = _build(lib, cfgs, sds)
    assert m.flow_incremental is False                                         # off by default
    plain = _tts(m, u)
    assert m.flow_passes == {"incremental": 0, "full": len(plain)} and m.flow.stat("stream_chunks") == 0
    m.flow_incremental = True
    m.flow_passes = {"incremental": 0, "full": 0}
    outs = _tts(m, u)
    assert [o.shape for o in outs] == [o.shape for o in plain] and len(outs) > 2
    tokens = OL.inference(sds[0], lc, u["text"], u["prompt_text"], u["llm_prompt_speech_token"])
    want = OM.Pipeline(sds, cfgs, token_hop_len=5, n_timesteps=2).tts(tokens, u, stream=True)
    assert len(outs) == len(want)
    for a, b in zip(outs, want):
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=0, atol=5e-3)                    # tests/test_model.py's waveform tolerance for the streamed request
    # every streaming chunk went through the request's stream, the last call (finalize=True) through the existing pass - counted, not timed
    assert m.flow_passes == {"incremental": len(outs) - 1, "full": 1}
    assert m.flow.stat("stream_chunks") == len(outs) - 1
    assert not m._flow_streams and m.flow.stat("open_streams") == 0 and m.flow.stat("stream_cache_bytes") == 0      # closed by tts()'s finally


def test_misaligned_chunk_falls_back_to_the_existing_pass(lib, setup):
    """A token count that is not chunk-aligned (2 * (8 + 11 - 3) = 32 frames against 10-frame chunks): the library refuses the call, the request drops its stream and
    token2wav is told to run the existing pass - for this chunk and for every later one of the request, aligned or not.  Another request is not affected."""
    cfgs, sds, u = setup
    lc, fc, hc = cfgs
    m = _build(lib, cfgs, sds)
    tok = torch.randint(0, fc.vocab, (1, 15), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    args = (u["flow_prompt_speech_token"], u["prompt_speech_feat"], u["flow_embedding"])
    with m._lane() as lane:
        assert m._flow_chunk_incremental(lane, tok[:, :11], *args, 0, "b") is None
        assert m._flow_streams == {"b": False} and m.flow.stat("open_streams") == 0
        assert m._flow_chunk_incremental(lane, tok, *args, 3, "b") is None                       # 40 frames: aligned, but the request has fallen back
        mel, skip = m._flow_chunk_incremental(lane, tok, *args, 0, "c")
        t = lambda n: torch.tensor([n], dtype=torch.int32)
        full, _ = lane.flow.inference(token=tok, token_len=t(15), prompt_token=args[0], prompt_token_len=t(8), prompt_feat=args[1], prompt_feat_len=t(16), embedding=args[2],
                                      streaming=True, finalize=False)
        assert skip == 0 and mel.shape == full.shape
        torch.testing.assert_close(mel.cpu(), full.cpu(), rtol=1e-4, atol=1e-4)
    assert m.flow_passes == {"incremental": 1, "full": 0} and m.flow.stat("open_streams") == 1
    m._close_flow_stream("c")
    m._close_flow_stream("b")
    assert not m._flow_streams and m.flow.stat("open_streams") == 0 and m.flow.stat("stream_cache_bytes") == 0
