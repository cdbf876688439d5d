"""Soft-capping (tfa_fwd_softcap / tfa_bwd_softcap) against the same calls without a cap, in one process, alternating.
Shapes: H32, bf16, D128 at 4 x 4096 and 1 x 16384; for each mask — causal and window (1024, 0) — three rows: no cap (tfa_fwd_local / tfa_bwd_local: the
existing kernels, which a causal window hands to tfa_fwd / tfa_bwd), softcap = 50, and softcap = 50 with the benchmark's ALiBi slopes.  Everything goes
through the C ABI with prebuilt parameter blocks; times are HIP events on the stream around `iters` back-to-back calls (after warm-up calls), best of
`--rounds` alternating rounds.  TFLOP/s counts the VISIBLE (query, key) pairs exactly — 4 * pairs * D * H * B for the forward, 2.5x that for the backward
(bench.py's convention); ratio = rate of the row / rate of the row of the same mask without a cap.
usage: python tools/bench_softcap.py [--ns 4096,16384] [--softcap 50] [--iters 10] [--rounds 3] [--no-bwd]"""
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
    ap.add_argument("--softcap", type=float, default=50.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bwd", action="store_true")
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    H, D, dtype = 32, 128, torch.bfloat16
    sc = 1.0 / math.sqrt(D)
    cap = a.softcap
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device=dev)
    sp = C.c_void_p(slopes.data_ptr())
    print(f"# softcap = {cap:g} vs no cap: H{H} D{D} bf16, causal and window (1024, 0), HIP events, best of {a.rounds} rounds x {a.iters} calls; "
          f"ratio = rate of the row / rate of the same mask without a cap")
    print(f"# {'shape':>10} {'mask':>10} {'softcap':>7} {'slopes':>6} {'fwd ms':>8} {'fwd TF':>7} {'ratio':>6} {'bwd ms':>8} {'bwd TF':>7} {'ratio':>6} {'kernel':>6}")
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
        # (window, capped, with slopes)
        arms = [(w, c, s) for w in ((-1, 0), (1024, 0)) for c, s in ((False, False), (True, False), (True, True))]

        def fcall(w, c, s):
            if c:
                return lambda: _lib.check(L.tfa_fwd_softcap(C.byref(pf), cap, sp if s else None, 0, w[0], w[1], stream))
            return lambda: _lib.check(L.tfa_fwd_local(C.byref(pf), w[0], w[1], stream))

        def bcall(w, c, s):
            if c:
                return lambda: _lib.check(L.tfa_bwd_softcap(C.byref(pb), cap, sp if s else None, 0, w[0], w[1], stream))
            return lambda: _lib.check(L.tfa_bwd_local(C.byref(pb), w[0], w[1], stream))

        best = {arm: [math.inf, math.inf] for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                f = fcall(*arm)
                best[arm][0] = min(best[arm][0], timeit(f, a.iters))
                if not a.no_bwd:
                    f()                              # (out / lse of this arm for its backward)
                    best[arm][1] = min(best[arm][1], timeit(bcall(*arm), a.iters))
        for w, c, s in arms:
            fl = 4.0 * B * H * visible_pairs(N, N, *w) * D
            f_ms, b_ms = best[(w, c, s)]
            f0, b0 = best[(w, False, False)]
            var = L.tfa_fwd_softcap_variant(C.byref(pf), cap, sp if s else None, 0, w[0], w[1]) if c else L.tfa_fwd_local_variant(C.byref(pf), w[0], w[1])
            name = "causal" if w == (-1, 0) else f"({w[0]},{w[1]})"
            print(f"  {B:>3}x{N:<6} {name:>10} {(f'{cap:g}' if c else 'no'):>7} {'yes' if s else 'no':>6} {f_ms:8.3f} {fl / f_ms / 1e9:7.1f} {f0 / f_ms:6.2f} "
                  f"{b_ms:8.3f} {2.5 * fl / b_ms / 1e9:7.1f} {(b0 / b_ms) if not a.no_bwd else float('nan'):6.2f} {var:>6}")


if __name__ == "__main__":
    main()
