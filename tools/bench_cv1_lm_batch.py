"""CosyVoice-300M TransformerLM at its real dimensions (configs.cv1(), synthetic weights) on the MI355X: 8 inference_sft-shaped greedy requests of the benchmark's token
budget (25 text tokens, 500 speech tokens each)
    A  through `inference` one after another (cv_lm1_decode: one weight stream per request and token - the only way before the batched decode),
    B  through `inference_batch(slots = 1 | 2 | 4 | 8)` (cv_lm1_batch_decode: one weight stream per lock-step step),
alternating A and B in ONE process, over fp32 and bf16 matrices.  Per run: wall time (prefills included - the same 8 in every run), decode steps, us per step, tokens / s.
Every request's ids in B must equal those in A: at full size that covers what the test shapes cannot (K = 4096, N = 4096, the 4097-row decoder).

    python tools/bench_cv1_lm_batch.py [--tokens 500] [--requests 8] [--reps 2] [--out profiles/cv1_lm_batch.json]
"""
import argparse
import json
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosyvoice_amd import cosyvoice1_hip as CK, synthetic as W   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=500)
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg, _ = W.cv1()
    sd = W.make_cv1_llm(cfg)
    n_text = 25
    g = torch.Generator().manual_seed(300)
    e0 = torch.zeros(1, 0, dtype=torch.int32)
    tl = lambda n: torch.tensor([n], dtype=torch.int32)
    ratio = args.tokens / n_text
    reqs = [dict(text=torch.randint(0, cfg.text_vocab, (1, n_text), generator=g, dtype=torch.int32), text_len=tl(n_text), prompt_text=e0, prompt_text_len=tl(0),
                 prompt_speech_token=e0, prompt_speech_token_len=tl(0), embedding=torch.randn(1, cfg.spk_dim, generator=g), max_token_text_ratio=ratio,
                 min_token_text_ratio=ratio) for _ in range(args.requests)]
    result = dict(tool="tools/bench_cv1_lm_batch.py", box=socket.gethostname(), device=torch.cuda.get_device_name(0), requests=args.requests, tokens_per_request=args.tokens,
                  n_text=n_text, note="wall times include the %d prefills of a run; us_per_step = wall / decode steps" % args.requests, modes={})
    for name, dtype in (("fp32", None), ("bf16", torch.bfloat16)):
        lm = CK.TransformerLM(sd, text_heads=cfg.text_heads, llm_heads=cfg.llm_heads, sampling="greedy", weight_dtype=dtype)

        def run_a():
            return [list(lm.inference(**r)) for r in reqs]

        def run_b(slots):
            got = [[] for _ in reqs]
            for i, toks in lm.inference_batch(reqs, slots=slots):
                got[i] += toks
            return got

        short = [dict(r, max_token_text_ratio=1, min_token_text_ratio=1) for r in reqs]      # warm-up: every kernel of both paths loaded before a clock starts
        for r in short[:1]:
            list(lm.inference(**r))
        for slots in (1, 2, 4, 8):
            list(lm.inference_batch(short, slots=slots))
        torch.cuda.synchronize()
        order = ["A", "B1", "B2", "B4", "B8"]
        runs, ids = [], {}
        for rep in range(args.reps):
            for label in (order if rep % 2 == 0 else ["A"] + order[:0:-1]):
                steps0 = lm.step_stat("steps") + lm.step_stat("batch_steps")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks = run_a() if label == "A" else run_b(int(label[1:]))
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                steps = lm.step_stat("steps") + lm.step_stat("batch_steps") - steps0
                n_tok = sum(len(x) for x in toks)
                ids.setdefault("A", toks)
                assert toks == ids["A"], "%s %s: the ids differ from the sequential run's" % (name, label)
                runs.append(dict(run=label, rep=rep, wall_s=round(wall, 4), steps=steps, us_per_step=round(1e6 * wall / max(steps, 1), 2), tokens=n_tok,
                                 tokens_per_s=round(n_tok / wall, 1)))
                print(name, runs[-1], flush=True)
        best = {}
        for r in runs:
            if r["run"] not in best or r["wall_s"] < best[r["run"]]["wall_s"]:
                best[r["run"]] = r
        a = best["A"]
        summary = {k: dict(us_per_step=v["us_per_step"], tokens_per_s=v["tokens_per_s"], speedup_vs_sequential=round(a["wall_s"] / v["wall_s"], 3),
                           step_cost_vs_1_slot=round(v["us_per_step"] / best["B1"]["us_per_step"], 3)) for k, v in best.items()}
        result["modes"][name] = dict(order=[r["run"] for r in runs], runs=runs, best=summary, ids_equal_sequential=True,
                                     slots1_vs_sequential_step=round(best["B1"]["us_per_step"] / a["us_per_step"], 4))
        del lm
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
