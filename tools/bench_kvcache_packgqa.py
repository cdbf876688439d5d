"""GQA packing of several rows per sequence in the K/V-cache call: tfa_fwd_kvcache_pack with TFA_PACK_GQA_OFF (unpacked: K / V streamed once per query head)
against TFA_PACK_GQA_ON (the packed form: once per K/V head), alternated in one process.  H32 Hk8 D128 bf16, causal, 16384 keys per sequence, Nq in {1, 2, 4, 8},
contiguous and paged (256) caches, 16-bit and e4m3; every arm runs the split count its own tfa_fwd_kvcache_pack_suggest_splits gives, and OFF is timed twice per
round (its repeat-to-repeat spread).  Through the C ABI with prebuilt parameter blocks; times are HIP events around `iters` back-to-back calls (after warm-up
calls), best of `--rounds` alternating rounds.  TB/s counts the K and V bytes of the actual lengths ONCE (2 * sum(len_b) * Hk * D * bytes per element): what a
call that streams each K/V head once has to move.
usage: python tools/bench_kvcache_packgqa.py [--bs 1,8,64] [--nqs 1,2,4,8] [--iters 10] [--rounds 3] [--out profiles/kvcache_packgqa_bench.txt]"""
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

H, HK, D, PAGE, NK = 32, 8, 128, 256, 16384
SCALE = 1.0 / math.sqrt(D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,8,64")
    ap.add_argument("--nqs", default="1,2,4,8")
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

    emit(f"# GQA packing at Nq >= 1 over a K/V cache: H{H} Hk{HK} D{D} bf16 causal, {NK} keys per sequence, page {PAGE}; tfa_fwd_kvcache_pack OFF vs ON, each at its own")
    emit(f"# suggested split count; HIP events, best of {a.rounds} rounds x {a.iters} calls, OFF / ON / OFF alternated; TB/s over the K/V bytes of the lengths, counted once")
    emit(f"# {'B':>3} {'Nq':>3} {'cache':>16} {'OFF s':>5} {'OFF ms':>8} {'TB/s':>6} {'OFF again':>9} {'ON s':>5} {'ON ms':>8} {'TB/s':>6} {'OFF/ON':>7}  note")
    for B in [int(x) for x in a.bs.split(",")]:
        kbuf = torch.empty((B, NK, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vbuf = torch.empty((B, NK, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        kd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.002, 0.02)
        vd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.002, 0.02)
        k8 = (kbuf.float() / kd.view(B, 1, HK, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
        v8 = (vbuf.float() / vd.view(B, 1, HK, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
        lens = torch.full((B,), NK, dtype=torch.int32, device=dev)
        mb = NK // PAGE
        bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
        p8 = _lib.TfaKvcacheFp8()
        p8.format = _lib.TFA_KV_E4M3
        p8.k_descale, p8.v_descale = kd.data_ptr(), vd.data_ptr()
        p8.k_descale_stride[0], p8.k_descale_stride[1] = kd.stride(0), kd.stride(1)
        p8.v_descale_stride[0], p8.v_descale_stride[1] = vd.stride(0), vd.stride(1)
        for Nq in [int(x) for x in a.nqs.split(",")]:
            q = torch.empty((B, Nq, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
            out = torch.empty((B, H, Nq, D), dtype=torch.bfloat16, device=dev)
            lse = torch.empty((B, H, Nq), dtype=torch.float32, device=dev)
            for fp8 in (False, True):
                for paged in (False, True):
                    kc, vc = (k8, v8) if fp8 else (kbuf, vbuf)
                    if paged:                                                         # the same storage seen as pages, reached through a shuffled table
                        kc, vc = kc.view(B * mb, PAGE, HK, D), vc.view(B * mb, PAGE, HK, D)
                    p = ops._kvcache_params(q, kc, vc, out, lse, lens, bt if paged else None, None, None, SCALE, True)
                    q8 = C.byref(p8) if fp8 else None
                    keep = []

                    def arm(mode):
                        s = L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(p), mode)
                        need = L.tfa_fwd_kvcache_pack_workspace(C.byref(p), q8, mode, s)
                        if need < 0:
                            _lib.check(int(need))
                        ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
                        keep.append(ws)
                        return (lambda: _lib.check(L.tfa_fwd_kvcache_pack(C.byref(p), q8, mode, s, ws.data_ptr(), stream))), s

                    f_off, s_off = arm(_lib.TFA_PACK_GQA_OFF)
                    f_on, s_on = arm(_lib.TFA_PACK_GQA_ON)
                    best = [math.inf, math.inf, math.inf]                             # OFF, ON, OFF again
                    for _ in range(a.rounds):
                        for i, f in enumerate((f_off, f_on, f_off)):
                            best[i] = min(best[i], timeit(f, a.iters))
                    kv_bytes = 2.0 * B * NK * HK * D * (1 if fp8 else 2)
                    off, on, off2 = best
                    tbs = lambda ms: kv_bytes / (ms * 1e-3) / 1e12
                    spread = abs(off - off2) / min(off, off2)
                    ratio = min(off, off2) / on
                    note = "ON slower than OFF beyond the repeat spread" if on > max(off, off2) * (1.0 + spread) else ""
                    name = f"{'e4m3' if fp8 else 'bf16'} {'paged' if paged else 'contiguous'}"
                    emit(f"  {B:3d} {Nq:3d} {name:>16} {s_off:5d} {off:8.4f} {tbs(off):6.2f} {off2:9.4f} {s_on:5d} {on:8.4f} {tbs(on):6.2f} {ratio:7.2f}  {note}")
                    del keep
        del kbuf, vbuf, k8, v8
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
