"""CosyVoice-300M's U-Net estimator at its real dimensions (configs.cv1(), synthetic weights) on the MI355X: the Euler solve of N in {1, 2, 4, 8} requests of about 500
speech tokens (861 mel frames, lengths spread +-15 %)
    A  as N single passes (EstimatorHandle.solve, cv_flow_solve: the only way before the padded pass),
    B  as ONE padded pass (EstimatorHandle.solve_batch, cv_flow_solve_ragged),
alternating A and B in one process after a warm-up of both, in fp32 and bf16 mode; per (mode, N) the median wall time of `--reps` runs of each (host clock around a
synchronised device: what a caller waits for).  Every request's mel in B must equal its mel in A bit for bit - at full size that covers C = 256 and the fused bf16
transformer kernels, which the test shapes (C = 32) do not reach.

    python tools/bench_cv1_flow_batch.py [--tokens 500] [--reps 5] [--steps 10] [--out profiles/cv1_flow_batch.txt]
"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosyvoice_amd import cosyvoice1_hip as CK, synthetic as W   # noqa: E402
from cosyvoice_amd._lib import get_lib                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg, _ = W.cv1()
    sd = W.make_cv1_flow(cfg)
    lib = get_lib()
    T0 = int(args.tokens / cfg.input_frame_rate * 22050 / 256)
    spread = [1.0, 0.85, 0.95, 0.90, 0.88, 0.97, 0.92, 0.86]        # the longest first: it sets Tmax at every N
    gen = torch.Generator().manual_seed(500)
    dev = torch.device("cuda")
    reqs = []
    for f in spread:
        L = int(T0 * f)
        reqs.append(tuple(torch.randn(L, 80, generator=gen).to(dev) for _ in range(3)) + (torch.randn(1, 80, generator=gen).to(dev),))      # z, mu, cond, spk
    lines = ["tool: tools/bench_cv1_flow_batch.py   box: %s   device: %s" % (socket.gethostname(), torch.cuda.get_device_name(0)),
             "requests of %d tokens -> %d frames, lengths x %s; %d Euler steps; median of %d runs each, A and B alternating; ms of wall time per run" %
             (args.tokens, T0, spread, args.steps, args.reps),
             "A = N x solve (one pass per request), B = one solve_batch (padded pass); ratio = A / B", ""]
    for precision in ("fp32", "bf16"):
        hd = CK.EstimatorHandle(sd, "decoder.estimator.", cfg.est_heads, lib, precision)
        for n in (1, 2, 4, 8):
            sub = reqs[:n]
            lens = [r[0].shape[0] for r in sub]
            Tmax = max(lens)
            pad = lambda k: torch.stack([torch.nn.functional.pad(r[k], (0, 0, 0, Tmax - r[k].shape[0])) for r in sub]).contiguous()
            z, mu, cond, spk = pad(0), pad(1), pad(2), torch.cat([r[3] for r in sub]).contiguous()

            def run_a():
                return [hd.solve(r[0].clone(), r[1], r[3], r[2], r[0].shape[0], args.steps) for r in sub]

            def run_b():
                return hd.solve_batch(z.clone(), mu, spk, cond, lens, args.steps)

            a, b = run_a(), run_b()                                  # warm-up of both paths at this shape, and the equality check
            torch.cuda.synchronize()
            equal = all(torch.equal(b[i, :lens[i]], a[i]) and (lens[i] == Tmax or float(b[i, lens[i]:].abs().max()) == 0.0) for i in range(n))
            assert equal, "%s N = %d: the padded pass differs from the single passes" % (precision, n)
            ta, tb = [], []
            for rep in range(args.reps):
                for which in (("A", "B") if rep % 2 == 0 else ("B", "A")):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run_a() if which == "A" else run_b()
                    torch.cuda.synchronize()
                    (ta if which == "A" else tb).append(1e3 * (time.perf_counter() - t0))
            ma, mb = statistics.median(ta), statistics.median(tb)
            lines.append("%s  N = %d  frames %s  A %8.2f ms (min %7.2f max %7.2f)   B %8.2f ms (min %7.2f max %7.2f)   ratio %5.2f   per request %7.2f -> %7.2f ms   bits equal: %s" %
                         (precision, n, lens, ma, min(ta), max(ta), mb, min(tb), max(tb), ma / mb, ma / n, mb / n, equal))
            print(lines[-1], flush=True)
        del hd
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
