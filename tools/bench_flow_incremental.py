"""Flow milliseconds per streaming chunk: the existing pass (flow.inference(streaming=True, finalize=False) over all tokens so far) against the incremental
stream (flow.open_stream().chunk(...): the Euler solve over the new frames only), full-size CosyVoice2 flow with synthetic weights, one request at a time.

Schedules: the model's own hop schedule (25, 50, then 100 tokens per hop, tts()) on a 75-token prompt for the 250-token U10 utterance and for a 750-token request.
Method: both paths on the same device in the same process, ALTERNATING round by round (a round = every chunk of the schedule on the existing pass, then the whole
schedule replayed on a fresh stream), WARM rounds first, then ROUNDS measured; a chunk's time is host wall time between two device synchronisations around the one call
(what token2wav waits for: enqueueing included), reported as the median and the minimum over the rounds.  The existing pass runs as the model runs it for a single
request (graph_max_rows = 1: issued launch by launch); the incremental path is never captured.  Then the incremental schedule again with 1 / 2 / 4 / 8 key slices of
the cached attention (cv_flow_stream_slices) - the table behind stream_slices_for() in csrc/flow.hip.

    python tools/bench_flow_incremental.py [--precision bf16|fp32] [--rounds 5] [--warm 2] [--out profiles/flow_incremental.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosyvoice_amd import synthetic as W
from cosyvoice_amd.flow import CausalMaskedDiffWithXvec

N_PROMPT, HOP, MAX_HOP = 75, 25, 100


def schedule(n_tokens, la):
    """new-token counts handed to token2wav by tts(stream=True): token_offset + hop + look-ahead, hop 25 -> 50 -> 100 -> 100 ..."""
    pad = -N_PROMPT % HOP
    out, off, hop = [], 0, HOP
    while True:
        this = hop + pad if off == 0 else hop
        if n_tokens - off < this + la:
            return out
        out.append(off + this + la)
        off += this
        hop = min(MAX_HOP, 2 * hop)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lc, fc, hc = W.cv2()
    flow = CausalMaskedDiffWithXvec(W.make_flow(fc), fc, precision=a.precision)
    flow.set_graph_rows(1)
    la = flow.pre_lookahead_len
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, fc.vocab, (1, N_PROMPT), generator=g, dtype=torch.int32)
    feat = torch.randn(1, 2 * N_PROMPT, 80, generator=g) * 2 - 5
    emb = torch.randn(1, fc.spk_dim, generator=g)
    t = lambda n: torch.tensor([n], dtype=torch.int32)
    say("flow ms per streaming chunk, %s mode, %d-token prompt, %d warm + %d measured alternating rounds, %s" % (a.precision, N_PROMPT, a.warm, a.rounds, torch.cuda.get_device_name(0)))
    for n_tokens in (250, 750):
        tok = torch.randint(0, fc.vocab, (1, n_tokens), generator=g, dtype=torch.int32)
        calls = schedule(n_tokens, la)
        T1 = [2 * (N_PROMPT + n - la) for n in calls]

        def full(n):
            return flow.inference(token=tok[:, :n], token_len=t(n), prompt_token=prompt, prompt_token_len=t(N_PROMPT), prompt_feat=feat, prompt_feat_len=t(2 * N_PROMPT),
                                  embedding=emb, streaming=True, finalize=False)[0]

        def replay():
            ms, mels = [], []
            with flow.open_stream(max_frames=T1[-1]) as st:
                for n in calls:
                    m_, mel = timed(lambda: st.chunk(tok[:, :n], prompt, feat, emb))
                    ms.append(m_); mels.append(mel)
                cache = flow.stat("stream_cache_bytes")
            return ms, mels, cache

        t_full, t_inc = [[] for _ in calls], [[] for _ in calls]
        worst, cache = 0.0, 0
        for rnd in range(a.warm + a.rounds):
            fulls = []
            for i, n in enumerate(calls):
                m_, mel = timed(lambda: full(n))
                fulls.append(mel)
                if rnd >= a.warm:
                    t_full[i].append(m_)
            ms, mels, cache = replay()
            done = 2 * N_PROMPT
            for i, (m_, mel) in enumerate(zip(ms, mels)):
                if rnd >= a.warm:
                    t_inc[i].append(m_)
                worst = max(worst, float((mel - fulls[i][:, :, done - 2 * N_PROMPT:]).abs().max()))
                done = T1[i]
        say()
        say("%d-token request: %d streaming chunks; caches at the last chunk %.2f GB; max |incremental - existing| over all returned frames %.3e" % (n_tokens, len(calls), cache / 2 ** 30, worst))
        say("chunk  frames so far  new frames | existing pass ms (median / min) | incremental ms (median / min) | incremental / existing")
        for i in range(len(calls)):
            new = T1[i] - (T1[i - 1] if i else 2 * N_PROMPT)
            mf, mi = statistics.median(t_full[i]), statistics.median(t_inc[i])
            say("%5d  %13d  %10d | %14.2f / %6.2f          | %12.2f / %6.2f         | %.2f%s" % (i, T1[i], new, mf, min(t_full[i]), mi, min(t_inc[i]), mi / mf,
                                                                                          "  faster" if mi < mf else "  not faster"))
        say("sum over the chunks: existing %.1f ms, incremental %.1f ms" % (sum(statistics.median(x) for x in t_full), sum(statistics.median(x) for x in t_inc)))
        if n_tokens == 750:
            say()
            say("key slices of the cached attention (cv_flow_stream_slices), incremental ms per chunk, median of %d replays after one warm replay; 0 = stream_slices_for()" % a.rounds)
            say("slices | " + " ".join("%7d" % k for k in T1) + "   (keys at the chunk)")
            for ns in (1, 2, 4, 8, 0):
                flow.lib.cv_flow_stream_slices(flow._h, C.c_int32(ns))
                replay()
                runs = [replay()[0] for _ in range(a.rounds)]
                say("%6d | " % ns + " ".join("%7.2f" % statistics.median(r[i] for r in runs) for i in range(len(calls))))
            flow.lib.cv_flow_stream_slices(flow._h, C.c_int32(0))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
