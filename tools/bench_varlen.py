"""Packed variable-length attention (tfa_fwd_varlen / tfa_bwd_varlen) against its two alternatives, in one process, alternating:
  varlen   one call over the packed batch (cu_seqlens on the device)
  padded   tfa_fwd / tfa_bwd on every sequence padded to the longest one ((B, max, H, D), bnhd views)
  loop     one tfa_fwd / tfa_bwd call per sequence
All three go through the C ABI with prebuilt parameter blocks; times are HIP events on the stream around `iters` back-to-back calls (after warm-up calls),
best of `--rounds` alternating rounds.  TFLOP/s counts ALGORITHMIC flops per sequence — 4 * visible (query, key) pairs * D * H, the exact pair count
under bottom-right causal masking — and 2.5x that for the backward (bench.py's convention), whatever the arm executes.  With --bwd the line also times
the zero-filled gradient tensors ops.flash_attn_varlen_bwd allocates around tfa_bwd_varlen (zero_fill_bwd), as a share of the C-ABI backward.
usage: python tools/bench_varlen.py [--mixes equal,pack,prefill] [--dims 128,64] [--iters 10] [--rounds 3] [--bwd]"""
import argparse
import ctypes as C
import math
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402


def mix_lengths(name, seed=0):
    r = random.Random(seed)
    if name == "equal":                              # the headline's shape as a packed batch: 4 x 4096
        return [4096] * 4
    if name == "pack":                               # training with sequence packing: documents of 512..8192 tokens fill rows of 16k tokens, 4 rows
        lens = []
        for _ in range(4):
            left = 16384
            while left > 0:
                n = min(left, r.randint(512, 8192))
                if left - n < 512:
                    n = left
                lens.append(n)
                left -= n
        return lens
    if name == "prefill":                            # prefill of mixed requests: many short prompts, a few long ones
        return [r.randint(32, 512) for _ in range(56)] + [r.randint(2048, 8192) for _ in range(4)]
    raise ValueError(name)


def visible_pairs(nq, nk, causal):
    if not causal:
        return nq * nk
    s = nk - nq                                      # row i sees keys 0 .. i + s
    return sum(max(0, min(nk, i + s + 1)) for i in range(nq))


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
    ap.add_argument("--mixes", default="equal,pack,prefill")
    ap.add_argument("--dims", default="128,64")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bwd", action="store_true", help="also time the backward of the three arms")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    dt, causal, H = torch.bfloat16, True, a.heads
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mix in a.mixes.split(","):
        lens = mix_lengths(mix)
        B, mx, tot = len(lens), max(lens), sum(lens)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
        for D in (int(d) for d in a.dims.split(",")):
            sc = 1.0 / math.sqrt(D)
            fl = 4.0 * H * D * sum(visible_pairs(n, n, causal) for n in lens)
            mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev).normal_(0, 0.5).to(dt)
            q, k, v, do = mk(tot, H, D), mk(tot, H, D), mk(tot, H, D), mk(tot, H, D)
            # varlen: the parameter blocks the ops build, reused
            out, lse = ops.flash_attn_varlen_fwd(q, k, v, cu, cu, mx, mx, causal, sc)
            pv = ops_varlen_params(q, k, v, out, lse, cu, mx, causal, sc)
            # padded: (B, max, H, D)
            qp, kp, vp, dop = (torch.zeros((B, mx, H, D), dtype=dt, device=dev) for _ in range(4))
            for b, n in enumerate(lens):
                o = int(cu[b])
                qp[b, :n], kp[b, :n], vp[b, :n], dop[b, :n] = q[o:o + n], k[o:o + n], v[o:o + n], do[o:o + n]
            outp, lsep = ops.flash_attn_fwd(qp, kp, vp, causal, sc, layout="bnhd")
            pp = ops.make_params(qp, kp, vp, outp, lsep, causal, sc, layout="bnhd")
            # loop: one problem per sequence (views into the packed tensors)
            loop = []
            for b, n in enumerate(lens):
                o = int(cu[b])
                qs, ks, vs, os_ = (t[o:o + n].unsqueeze(0) for t in (q, k, v, out))
                ls = torch.empty((1, H, n), dtype=torch.float32, device=dev)
                loop.append((ops.make_params(qs, ks, vs, os_, ls, causal, sc, layout="bnhd"), ls))
            arms = {"varlen": lambda: _lib.check(L.tfa_fwd_varlen(C.byref(pv), st)),
                    "padded": lambda: _lib.check(L.tfa_fwd(C.byref(pp), st)),
                    "loop": lambda: [_lib.check(L.tfa_fwd(C.byref(p_), st)) for p_, _ in loop]}
            if a.bwd:
                vb = ops_varlen_bwd_params(q, k, v, out, lse, do, cu, mx, causal, sc, dev)
                gp = [torch.empty_like(qp), torch.empty_like(kp), torch.empty_like(vp), torch.empty_like(lsep)]
                pbp = ops.make_bwd_params(qp, kp, vp, outp, lsep, dop, gp[0], gp[1], gp[2], gp[3], causal, sc, layout="bnhd")
                lb = []
                for b, n in enumerate(lens):
                    o = int(cu[b])
                    views = [t[o:o + n].unsqueeze(0) for t in (q, k, v, out, do)]
                    ls = torch.empty((1, H, n), dtype=torch.float32, device=dev)
                    pf = ops.make_params(views[0], views[1], views[2], views[3], ls, causal, sc, layout="bnhd")
                    _lib.check(L.tfa_fwd(C.byref(pf), st))
                    g = [torch.empty_like(views[0]), torch.empty_like(views[1]), torch.empty_like(views[2]), torch.empty_like(ls)]
                    lb.append((ops.make_bwd_params(views[0], views[1], views[2], views[3], ls, views[4], g[0], g[1], g[2], g[3], causal, sc, layout="bnhd"), g, ls))
                arms["varlen_bwd"] = lambda: _lib.check(L.tfa_bwd_varlen(C.byref(vb[0]), st))
                arms["padded_bwd"] = lambda: _lib.check(L.tfa_bwd(C.byref(pbp), st))
                arms["loop_bwd"] = lambda: [_lib.check(L.tfa_bwd(C.byref(p_), st)) for p_, _, _ in lb]
                # what ops.flash_attn_varlen_bwd adds on top of tfa_bwd_varlen: its three zero-filled gradient tensors (the kernels never write the rows
                # outside every sequence); allocations come from torch's caching allocator, so this is the three memsets
                arms["zero_fill_bwd"] = lambda: (torch.zeros(q.shape, dtype=dt, device=dev), torch.zeros(k.shape, dtype=dt, device=dev),
                                                 torch.zeros(v.shape, dtype=dt, device=dev))
            best = {n: float("inf") for n in arms}
            for _ in range(a.rounds):
                for n, fn in arms.items():
                    best[n] = min(best[n], timeit(fn, a.iters))
            padded_fl = 4.0 * H * D * B * visible_pairs(mx, mx, causal)
            print(f"{mix:8s} D{D:<3d} B{B:<3d} tokens {tot:6d} max {mx:5d} H{H} bf16 causal  padded/real flops {padded_fl / fl:5.2f}x  |  " +
                  "  ".join(f"{n} {ms:8.3f} ms" + ("" if n.startswith("zero") else f" {(2.5 if n.endswith('bwd') else 1.0) * fl / ms / 1e9:7.1f} TF")
                            for n, ms in best.items()) +
                  f"  |  padded/varlen {best['padded'] / best['varlen']:.2f}x  loop/varlen {best['loop'] / best['varlen']:.2f}x" +
                  (f"  bwd: padded/varlen {best['padded_bwd'] / best['varlen_bwd']:.2f}x  loop/varlen {best['loop_bwd'] / best['varlen_bwd']:.2f}x"
                   f"  zero-fill/varlen_bwd {100.0 * best['zero_fill_bwd'] / best['varlen_bwd']:.1f} %" if a.bwd else ""),
                  flush=True)


def ops_varlen_params(q, k, v, out, lse, cu, mx, causal, sc):
    p = _lib.TfaVarlenFwdParams()
    p.q, p.k, p.v, p.out, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    p.cu_seqlens_q = p.cu_seqlens_k = cu.data_ptr()
    p.B, p.H, p.Hk, p.D = cu.numel() - 1, q.shape[1], k.shape[1], q.shape[2]
    p.max_seqlen_q = p.max_seqlen_k = mx
    p.total_q, p.total_k = q.shape[0], k.shape[0]
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out)):
        getattr(p, name)[0], getattr(p, name)[1] = t.stride(1), t.stride(0)
    p.softmax_scale, p.is_causal = sc, int(causal)
    p.dtype = p.out_dtype = _lib.TFA_BF16 if q.dtype == torch.bfloat16 else _lib.TFA_F16
    return p


def ops_varlen_bwd_params(q, k, v, out, lse, do, cu, mx, causal, sc, dev):
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty_like(lse)
    p = _lib.TfaVarlenBwdParams()
    p.q, p.k, p.v, p.out, p.dout, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr()
    p.dq, p.dk, p.dv, p.delta = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    p.cu_seqlens_q = p.cu_seqlens_k = cu.data_ptr()
    p.B, p.H, p.Hk, p.D = cu.numel() - 1, q.shape[1], k.shape[1], q.shape[2]
    p.max_seqlen_q = p.max_seqlen_k = mx
    p.total_q, p.total_k = q.shape[0], k.shape[0]
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out), ("do_stride", do), ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv)):
        getattr(p, name)[0], getattr(p, name)[1] = t.stride(1), t.stride(0)
    p.softmax_scale, p.is_causal = sc, int(causal)
    p.dtype = p.grad_dtype = _lib.TFA_BF16 if q.dtype == torch.bfloat16 else _lib.TFA_F16
    return p, (dq, dk, dv, delta)


if __name__ == "__main__":
    main()
