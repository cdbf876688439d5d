"""ALiBi (tfa_fwd_alibi / tfa_bwd_alibi) against the same calls without slopes, in one process, alternating.
Shapes: H32, bf16, D128 at 4 x 4096 and 1 x 16384; pairs: causal without slopes (tfa_fwd / tfa_bwd: the existing kernels) and with slopes, window
(1024, 0) without slopes (tfa_fwd_local / tfa_bwd_local) and with.  Everything goes through the C ABI with prebuilt parameter blocks; times are HIP
events on the stream around `iters` back-to-back calls (after warm-up calls), best of `--rounds` alternating rounds.  TFLOP/s counts the VISIBLE
(query, key) pairs exactly — 4 * pairs * D * H * B for the forward, 2.5x that for the backward (bench.py's convention).
usage: python tools/bench_alibi.py [--ns 4096,16384] [--iters 10] [--rounds 3] [--no-bwd]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402
from tools.bench_window import timeit, visible_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="4096,16384")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bwd", action="store_true")
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    H, D, dtype = 32, 128, torch.bfloat16
    sc = 1.0 / math.sqrt(D)
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device=dev)
    sp = C.c_void_p(slopes.data_ptr())
    print(f"# ALiBi vs no slopes: H{H} D{D} bf16, causal and window (1024, 0), HIP events, best of {a.rounds} rounds x {a.iters} calls; ratio = rate with / rate without slopes")
    print(f"# {'shape':>10} {'mask':>10} {'slopes':>6} {'fwd ms':>8} {'fwd TF':>7} {'ratio':>6} {'bwd ms':>8} {'bwd TF':>7} {'ratio':>6} {'kernel':>6}")
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
        arms = [((-1, 0), False), ((-1, 0), True), ((1024, 0), False), ((1024, 0), True)]

        def fcall(w, al):
            if al:
                return lambda: _lib.check(L.tfa_fwd_alibi(C.byref(pf), sp, 0, w[0], w[1], stream))
            return lambda: _lib.check(L.tfa_fwd_local(C.byref(pf), w[0], w[1], stream))

        def bcall(w, al):
            if al:
                return lambda: _lib.check(L.tfa_bwd_alibi(C.byref(pb), sp, 0, w[0], w[1], stream))
            return lambda: _lib.check(L.tfa_bwd_local(C.byref(pb), w[0], w[1], stream))

        best = {arm: [math.inf, math.inf] for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                f = fcall(*arm)
                best[arm][0] = min(best[arm][0], timeit(f, a.iters))
                if not a.no_bwd:
                    f()                              # (out / lse of this arm for its backward)
                    best[arm][1] = min(best[arm][1], timeit(bcall(*arm), a.iters))
        for w, al in arms:
            fl = 4.0 * B * H * visible_pairs(N, N, *w) * D
            f_ms, b_ms = best[(w, al)]
            f0, b0 = best[(w, False)]
            var = L.tfa_fwd_alibi_variant(C.byref(pf), sp, 0, w[0], w[1]) if al else L.tfa_fwd_local_variant(C.byref(pf), w[0], w[1])
            name = "causal" if w == (-1, 0) else f"({w[0]},{w[1]})"
            print(f"  {B:>3}x{N:<6} {name:>10} {'yes' if al else 'no':>6} {f_ms:8.3f} {fl / f_ms / 1e9:7.1f} {f0 / f_ms:6.2f} "
                  f"{b_ms:8.3f} {2.5 * fl / b_ms / 1e9:7.1f} {(b0 / b_ms) if not a.no_bwd else float('nan'):6.2f} {var:>6}")


if __name__ == "__main__":
    main()
