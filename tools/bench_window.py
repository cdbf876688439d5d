"""Local (sliding-window) attention (tfa_fwd_local / tfa_bwd_local) against full causal attention on the same shapes, in one process, alternating.
Shapes: H32, bf16, D128, causal, N = 16384 (B1) and 4096 (B4), windows left in {256, 1024, 4096} and full causal (-1, 0).  Everything goes through
the C ABI with prebuilt parameter blocks; times are HIP events on the stream around `iters` back-to-back calls (after warm-up calls), best of
`--rounds` alternating rounds.  TFLOP/s counts the VISIBLE (query, key) pairs exactly — 4 * pairs * D * H * B for the forward, 2.5x that for the
backward (bench.py's convention) — computed from the shapes, so a window's rate is comparable with full causal attention's.
usage: python tools/bench_window.py [--ns 16384,4096] [--lefts 256,1024,4096] [--iters 10] [--rounds 3] [--no-bwd]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402


def visible_pairs(nq, nk, left, right):
    """Exact count of (i, j) with max(0, i + s - left) <= j <= min(nk - 1, i + s + right), s = nk - nq (-1 = unbounded)."""
    s, tot = nk - nq, 0
    for i in range(nq):
        lo = 0 if left < 0 else max(0, i + s - left)
        hi = nk - 1 if right < 0 else min(nk - 1, i + s + right)
        tot += max(0, hi - lo + 1)
    return tot


def timeit(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="16384,4096")
    ap.add_argument("--lefts", default="256,1024,4096")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bwd", action="store_true")
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    H, D, dtype = 32, 128, torch.bfloat16
    sc = 1.0 / math.sqrt(D)
    print(f"# local attention vs full causal: H{H} D{D} bf16, causal, HIP events, best of {a.rounds} rounds x {a.iters} calls")
    print(f"# {'shape':>10} {'window':>10} {'fwd ms':>8} {'fwd TF':>7} {'x causal':>8} {'bwd ms':>8} {'bwd TF':>7} {'x causal':>8} {'pairs':>14} {'kernel':>6}")
    for N in [int(x) for x in a.ns.split(",")]:
        B = max(1, 16384 // N)
        g = torch.Generator(device=dev).manual_seed(0)
        q, k, v, dout = (torch.randn((B, H, N, D), generator=g, device=dev, dtype=torch.float32).mul_(0.5).to(dtype) for _ in range(4))
        out = torch.empty_like(q)
        lse = torch.empty((B, H, N), dtype=torch.float32, device=dev)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        pf = ops.make_params(q, k, v, out, lse, True, sc)
        pb = ops.make_bwd_params(q, k, v, out, lse, dout, dq, dk, dv, delta, True, sc)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        windows = [(-1, 0)] + [(int(x), 0) for x in a.lefts.split(",")]
        best = {w: [math.inf, math.inf] for w in windows}
        for _ in range(a.rounds):
            for w in windows:
                f = lambda w=w: _lib.check(L.tfa_fwd_local(C.byref(pf), w[0], w[1], stream))   # noqa: E731
                best[w][0] = min(best[w][0], timeit(f, a.iters))
                if not a.no_bwd:
                    f()
                    bk = lambda w=w: _lib.check(L.tfa_bwd_local(C.byref(pb), w[0], w[1], stream))   # noqa: E731
                    best[w][1] = min(best[w][1], timeit(bk, a.iters))
        for w in windows:
            pairs = B * H * visible_pairs(N, N, *w)
            fl = 4.0 * pairs * D
            f_ms, b_ms = best[w]
            fx = best[(-1, 0)][0] / f_ms
            bx = best[(-1, 0)][1] / b_ms if not a.no_bwd else float("nan")
            name = "causal" if w == (-1, 0) else f"({w[0]},{w[1]})"
            print(f"  {B:>3}x{N:<6} {name:>10} {f_ms:8.3f} {fl / f_ms / 1e9:7.1f} {fx:8.2f} {b_ms:8.3f} {2.5 * fl / b_ms / 1e9:7.1f} {bx:8.2f} "
                  f"{pairs:14d} {L.tfa_fwd_local_variant(C.byref(pf), w[0], w[1]):>6}")


if __name__ == "__main__":
    main()
