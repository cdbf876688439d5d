"""The dense bias (tfa_fwd_bias / tfa_bwd_bias) against the same calls without one, in one process, alternating.
Shapes: H32, bf16, D128 at 4 x 4096 and 1 x 16384, causal and full.  Arms per shape and mask: no bias (tfa_fwd_local / tfa_bwd_local for the same mask),
a (B,H,Nq,Nk) bf16 bias, a (1,H,Nq,Nk) bf16 bias, a (1,1,Nq,Nk) bf16 bias and an fp32 (B,H,Nq,Nk) bias; forward and backward.  Everything goes through
the C ABI with prebuilt parameter blocks; times are HIP events on the stream around `iters` back-to-back calls (after warm-up calls), best of `--rounds`
alternating rounds.  There is no pass bar on speed: a full-shape bias is B * H * Nq * Nk * esize bytes that must come from HBM once per forward and twice
per backward (the dQ and the dK/dV launch each read it) — the `floor` columns are those bytes over the HBM rate bench.py uses (PEAK_HBM_GBS); a broadcast
bias is re-read from the caches and its floor counts the distinct bytes once.  A causal mask visits half of the tiles: its floor counts half of the bytes.
The table goes to stdout and to profiles/bias_bench.txt.
usage: python tools/bench_bias.py [--ns 4096,16384] [--iters 10] [--rounds 3] [--no-bwd] [--out profiles/bias_bench.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402
from bench import PEAK_HBM_GBS  # noqa: E402
from tools.bench_window import timeit, visible_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="4096,16384")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bwd", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_bench.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    H, D, dtype = 32, 128, torch.bfloat16
    sc = 1.0 / math.sqrt(D)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# dense bias vs no bias: H{H} D{D} bf16, HIP events, best of {a.rounds} rounds x {a.iters} calls; floor = distinct bias bytes the mask visits / "
         f"{PEAK_HBM_GBS / 1000:.0f} TB/s (x2 for the backward); ratio = time without / time with the bias")
    emit(f"# {'shape':>10} {'mask':>7} {'bias':>14} {'fwd ms':>8} {'floor':>7} {'fwd TF':>7} {'ratio':>6} {'bwd ms':>8} {'floor':>7} {'bwd TF':>7} {'ratio':>6} {'kernel':>6}")
    for N in [int(x) for x in a.ns.split(",")]:
        B = max(1, 16384 // N)
        g = torch.Generator(device=dev).manual_seed(0)
        q, k, v, dout = (torch.randn((B, H, N, D), generator=g, device=dev, dtype=torch.float32).mul_(0.5).to(dtype) for _ in range(4))
        out = torch.empty_like(q)
        lse = torch.empty((B, H, N), dtype=torch.float32, device=dev)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        kinds = [("none", None, None), ("(B,H) bf16", (B, H), dtype), ("(1,H) bf16", (1, H), dtype), ("(1,1) bf16", (1, 1), dtype), ("(B,H) fp32", (B, H), torch.float32)]
        for causal in (True, False):
            w = (-1, 0) if causal else (-1, -1)
            pf = ops.make_params(q, k, v, out, lse, causal, sc)
            pb = ops.make_bwd_params(q, k, v, out, lse, dout, dq, dk, dv, delta, causal, sc)
            best, floors, variants = {}, {}, {}
            for name, shape, bdt in kinds:          # (one bias tensor alive at a time: the fp32 one is 34 GB at 1 x 16384)
                bias = st = None
                if shape is not None:
                    bias = torch.empty((shape[0], shape[1], N, N), dtype=bdt, device=dev)
                    for b in range(shape[0]):       # (filled slice by slice: no fp32 temporary of the whole tensor)
                        bias[b].normal_(0.0, 1.0, generator=g)
                    _, st = ops._attn_bias(bias, B, H, N, N, dev, dtype, D)
                    fcall = lambda: _lib.check(L.tfa_fwd_bias(C.byref(pf), C.byref(st), w[0], w[1], stream))      # noqa: E731
                    bcall = lambda: _lib.check(L.tfa_bwd_bias(C.byref(pb), C.byref(st), w[0], w[1], stream))      # noqa: E731
                    variants[name] = L.tfa_fwd_bias_variant(C.byref(pf), C.byref(st), w[0], w[1])
                    floors[name] = bias.numel() * bias.element_size() * (0.5 if causal else 1.0) / (PEAK_HBM_GBS * 1e9) * 1e3
                else:
                    fcall = lambda: _lib.check(L.tfa_fwd_local(C.byref(pf), w[0], w[1], stream))                  # noqa: E731
                    bcall = lambda: _lib.check(L.tfa_bwd_local(C.byref(pb), w[0], w[1], stream))                  # noqa: E731
                    variants[name] = L.tfa_fwd_local_variant(C.byref(pf), w[0], w[1])
                    floors[name] = 0.0
                best[name] = [math.inf, math.inf]
                for _ in range(a.rounds):
                    best[name][0] = min(best[name][0], timeit(fcall, a.iters))
                    if not a.no_bwd:
                        fcall()                      # (out / lse of this arm for its backward)
                        best[name][1] = min(best[name][1], timeit(bcall, a.iters))
                del bias, st
                torch.cuda.empty_cache()
            fl = 4.0 * B * H * visible_pairs(N, N, *w) * D
            for name, _, _ in kinds:
                f_ms, b_ms = best[name]
                f0, b0 = best["none"]
                emit(f"  {B:>3}x{N:<6} {'causal' if causal else 'full':>7} {name:>14} {f_ms:8.3f} {floors[name]:7.3f} {fl / f_ms / 1e9:7.1f} {f0 / f_ms:6.2f} "
                     f"{b_ms:8.3f} {2 * floors[name]:7.3f} {2.5 * fl / b_ms / 1e9:7.1f} {(b0 / b_ms) if not a.no_bwd else float('nan'):6.2f} {variants[name]:>6}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
