"""Decode over a K/V cache: tfa_fwd_kvcache (device-side lengths, contiguous and paged, with and without the in-place append) against what a caller had before
it — tfa_fwd_splitkv on equal lengths (the baseline, run twice: its own repeat-to-repeat spread), the ragged batch padded to its longest sequence (WRONG
results: the padding is attended), and a host loop of one call per sequence.  H32 Hk8 D128 bf16, Nq = 1, through the C ABI with prebuilt parameter blocks;
times are HIP events around `iters` back-to-back calls (after warm-up calls), best of `--rounds` alternating rounds.  TB/s counts the K and V bytes of the
ACTUAL lengths once (2 * sum(len_b) * Hk * D * 2 bytes).
usage: python tools/bench_kvcache.py [--bs 1,8,64] [--iters 10] [--rounds 3] [--out profiles/kvcache_bench.txt]"""
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


def fwd_params(q, kc, vc, out, lse, B, nk):
    """tfa_fwd_params of a decode step over the first nk keys of (B', cap, Hk, D) caches: q (B, 1, H, D), out dense (B, H, 1, D)."""
    p = _lib.TfaFwdParams()
    p.q, p.k, p.v, p.out, p.lse = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), lse.data_ptr()
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, HK, 1, nk, D
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = q.stride(0), q.stride(2), q.stride(1)
    for name, t in (("k_stride", kc), ("v_stride", vc)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * D, D, D
    p.softmax_scale = SCALE
    p.is_causal = 0
    p.dtype = p.out_dtype = _lib.TFA_BF16
    return p


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

    emit(f"# decode over a K/V cache: H{H} Hk{HK} D{D} bf16 Nq1, page {PAGE}, HIP events, best of {a.rounds} rounds x {a.iters} calls; TB/s over the K/V bytes of the actual lengths")
    emit(f"# {'B':>3} {'lengths':>22} {'path':>34} {'splits':>6} {'ms':>8} {'TB/s':>6} {'+append ms':>10} {'TB/s':>6}  note")
    for B in [int(x) for x in a.bs.split(",")]:
        gen = torch.Generator().manual_seed(1234 + B)
        ragged = torch.randint(1024, 32768 + 1, (B,), generator=gen).to(torch.int32)
        cap_max = 32768
        kbuf = torch.empty((B, cap_max, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vbuf = torch.empty((B, cap_max, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        q = torch.empty((B, 1, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        kn = torch.empty((B, 1, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vn = torch.empty((B, 1, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        out = torch.empty((B, H, 1, D), dtype=torch.bfloat16, device=dev)
        lse = torch.empty((B, H, 1), dtype=torch.float32, device=dev)
        keep = []                                                                     # workspaces and tables stay alive while their calls are timed

        def splitkv_call(p):
            s = L.tfa_fwd_suggest_splits(C.byref(p))
            if s < 2:
                return (lambda: _lib.check(L.tfa_fwd(C.byref(p), stream))), 1
            ws = torch.empty((int(L.tfa_fwd_splitkv_workspace(C.byref(p), s)),), dtype=torch.float32, device=dev)
            keep.append(ws)
            return (lambda: _lib.check(L.tfa_fwd_splitkv(C.byref(p), s, ws.data_ptr(), stream))), s

        def kvcache_call(lens, cap, paged, append):
            kc, vc = kbuf[:, :cap], vbuf[:, :cap]
            lens_dev = (lens - (1 if append else 0)).to(dev)
            keep.append(lens_dev)
            bt = None
            if paged:                                                                 # the same storage seen as pages, reached through a shuffled table
                mb = cap_max // PAGE
                perm = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb)[:, : cap // PAGE].contiguous()
                bt = perm.to(torch.int32).to(dev)
                keep.append(bt)
                kc, vc = kbuf.view(B * mb, PAGE, HK, D), vbuf.view(B * mb, PAGE, HK, D)
            p = ops._kvcache_params(q, kc, vc, out, lse, lens_dev, bt, kn if append else None, vn if append else None, SCALE, False)
            s = L.tfa_fwd_kvcache_suggest_splits(C.byref(p))
            need = L.tfa_fwd_kvcache_workspace(C.byref(p), s)
            if need < 0:
                _lib.check(int(need))
            ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
            keep.extend([ws, p])
            return (lambda: _lib.check(L.tfa_fwd_kvcache(C.byref(p), s, ws.data_ptr(), stream))), s

        for label, lens, cap in (("equal 16384", torch.full((B,), 16384, dtype=torch.int32), 16384),
                                 (f"ragged [{int(ragged.min())}, {int(ragged.max())}]", ragged, cap_max)):
            kv_bytes = 2.0 * float(lens.sum()) * HK * D * 2
            arms = []                                                                 # (path, call, splits, append call or None, note)
            if cap == 16384:
                p0 = fwd_params(q, kbuf, vbuf, out, lse, B, 16384)
                keep.append(p0)
                for rep in (1, 2):
                    f, s = splitkv_call(p0)
                    arms.append((f"tfa_fwd_splitkv (baseline, run {rep})", f, s, None, ""))
            for paged in (False, True):
                f, s = kvcache_call(lens, cap, paged, False)
                fa, _ = kvcache_call(lens, cap, paged, True)
                arms.append((f"tfa_fwd_kvcache {'paged' if paged else 'contiguous'}", f, s, fa, ""))
            if cap != 16384:
                nmax = int(lens.max())
                pp = fwd_params(q, kbuf, vbuf, out, lse, B, nmax)
                keep.append(pp)
                f, s = splitkv_call(pp)
                arms.append((f"padded to {nmax}: tfa_fwd_splitkv", f, s, None, "WRONG RESULTS (padding attended)"))
                calls = []
                for b in range(B):
                    pb = fwd_params(q[b:b + 1], kbuf[b:b + 1], vbuf[b:b + 1], out[b:b + 1], lse[b:b + 1], 1, int(lens[b]))
                    keep.append(pb)
                    calls.append(splitkv_call(pb)[0])
                arms.append((f"host loop: {B} x tfa_fwd_splitkv", (lambda cs=calls: [c() for c in cs]), 0, None, "one call (+ merge) per sequence"))
            best = [[math.inf, math.inf] for _ in arms]
            for _ in range(a.rounds):
                for i, (_, f, _, fa, _) in enumerate(arms):
                    best[i][0] = min(best[i][0], timeit(f, a.iters))
                    if fa is not None:
                        best[i][1] = min(best[i][1], timeit(fa, a.iters))
            for (name, _, s, fa, note), (ms, msa) in zip(arms, best):
                app = f"{msa:10.4f} {kv_bytes / (msa * 1e-3) / 1e12:6.2f}" if fa is not None else f"{'-':>10} {'-':>6}"
                emit(f"  {B:3d} {label:>22} {name:>34} {s if s else '-':>6} {ms:8.4f} {kv_bytes / (ms * 1e-3) / 1e12:6.2f} {app}  {note}")
        del kbuf, vbuf, keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
