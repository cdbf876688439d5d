"""Decode over an fp8 (e4m3) K/V cache: tfa_fwd_kvcache_fp8 against the 16-bit tfa_fwd_kvcache on the same lengths, in the same process.  H32 Hk8 D128, q / out
bf16, Nq = 1, B in {1, 8, 64}: equal lengths 16384 and the ragged batch of tools/bench_kvcache.py (same seed), contiguous and paged, through the C ABI with
prebuilt parameter blocks.  The 16-bit call is the baseline and runs TWICE per row (its own repeat-to-repeat spread); both calls take the split count the library
suggests (one rule for both cache types).  Times are HIP events around `iters` back-to-back calls, best of `--rounds` alternating rounds.  TB/s counts the K and V
bytes each path actually streams: 2 * sum(len_b) * Hk * D * (2 or 1) bytes.  ratio = fp8 ms / 16-bit ms (best of the two baseline runs); "+append" is the same call
with one new row per sequence quantised and appended first (its extra cost over the plain call is the append's launch).
usage: python tools/bench_kvcache_fp8.py [--bs 1,8,64] [--iters 10] [--rounds 3] [--out profiles/kvcache_fp8_bench.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402
from tools.bench_window import timeit  # noqa: E402

H, HK, D, PAGE = 32, 8, 128, 256
SCALE = 1.0 / math.sqrt(D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,8,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# decode over a K/V cache, 16-bit against fp8 (e4m3): H{H} Hk{HK} D{D} q/out bf16 Nq1, page {PAGE}, HIP events, best of {a.rounds} rounds x {a.iters} calls")
    emit("# TB/s over the K/V bytes each path streams; ratio = fp8 ms / best 16-bit ms")
    emit(f"# {'B':>3} {'lengths':>22} {'layout':>10} {'splits':>6} | {'16-bit ms':>9} {'run 2':>8} {'TB/s':>6} | {'fp8 ms':>8} {'TB/s':>6} {'ratio':>6} | {'fp8 +append ms':>14} {'16-bit +append':>14}")
    for B in [int(x) for x in a.bs.split(",")]:
        gen = torch.Generator().manual_seed(1234 + B)
        ragged = torch.randint(1024, 32768 + 1, (B,), generator=gen).to(torch.int32)
        cap_max = 32768
        kbuf = torch.empty((B, cap_max, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vbuf = torch.empty((B, cap_max, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        kd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.002, 0.02)
        vd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.002, 0.02)
        k8 = (kbuf.float() / kd.view(B, 1, HK, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
        v8 = (vbuf.float() / vd.view(B, 1, HK, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
        q = torch.empty((B, 1, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        kn = torch.empty((B, 1, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vn = torch.empty((B, 1, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        out = torch.empty((B, H, 1, D), dtype=torch.bfloat16, device=dev)
        lse = torch.empty((B, H, 1), dtype=torch.float32, device=dev)
        keep = []                                                                     # workspaces, tables and parameter blocks stay alive while their calls are timed

        def call(fp8, lens, cap, paged, append):
            kb, vb = (k8, v8) if fp8 else (kbuf, vbuf)
            kc, vc = kb[:, :cap], vb[:, :cap]
            lens_dev = (lens - (1 if append else 0)).to(dev)
            bt = None
            if paged:                                                                 # the same storage seen as pages, reached through a shuffled table
                mb = cap_max // PAGE
                perm = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb)[:, : cap // PAGE].contiguous()
                bt = perm.to(torch.int32).to(dev)
                kc, vc = kb.view(B * mb, PAGE, HK, D), vb.view(B * mb, PAGE, HK, D)
            p = ops._kvcache_params(q, kc, vc, out, lse, lens_dev, bt, kn if append else None, vn if append else None, SCALE, False)
            s = L.tfa_fwd_kvcache_suggest_splits(C.byref(p))
            p8 = _lib.TfaKvcacheFp8()
            p8.format = _lib.TFA_KV_E4M3
            p8.k_descale, p8.v_descale = kd.data_ptr(), vd.data_ptr()
            p8.k_descale_stride[0], p8.k_descale_stride[1] = kd.stride(0), kd.stride(1)
            p8.v_descale_stride[0], p8.v_descale_stride[1] = vd.stride(0), vd.stride(1)
            need = L.tfa_fwd_kvcache_fp8_workspace(C.byref(p), C.byref(p8), s) if fp8 else L.tfa_fwd_kvcache_workspace(C.byref(p), s)
            if need < 0:
                _lib.check(int(need))
            ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
            keep.extend([ws, p, p8, lens_dev, bt])
            if fp8:
                return (lambda: _lib.check(L.tfa_fwd_kvcache_fp8(C.byref(p), C.byref(p8), s, ws.data_ptr(), stream))), s
            return (lambda: _lib.check(L.tfa_fwd_kvcache(C.byref(p), s, ws.data_ptr(), stream))), s

        for label, lens, cap in (("equal 16384", torch.full((B,), 16384, dtype=torch.int32), 16384),
                                 (f"ragged [{int(ragged.min())}, {int(ragged.max())}]", ragged, cap_max)):
            elems = 2.0 * float(lens.sum()) * HK * D
            for paged in (False, True):
                f16, s = call(False, lens, cap, paged, False)
                f16b, _ = call(False, lens, cap, paged, False)
                f8, s8 = call(True, lens, cap, paged, False)
                f16a, _ = call(False, lens, cap, paged, True)
                f8a, _ = call(True, lens, cap, paged, True)
                assert s == s8
                arms = [f16, f16b, f8, f16a, f8a]
                best = [math.inf] * len(arms)
                for _ in range(a.rounds):
                    for i, f in enumerate(arms):
                        best[i] = min(best[i], timeit(f, a.iters))
                t16 = min(best[0], best[1])
                emit(f"  {B:3d} {label:>22} {'paged' if paged else 'contiguous':>10} {s:6d} | {best[0]:9.4f} {best[1]:8.4f} {elems * 2 / (t16 * 1e-3) / 1e12:6.2f} | "
                     f"{best[2]:8.4f} {elems / (best[2] * 1e-3) / 1e12:6.2f} {best[2] / t16:6.3f} | {best[4]:14.4f} {best[3]:14.4f}")
        del kbuf, vbuf, k8, v8, keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
