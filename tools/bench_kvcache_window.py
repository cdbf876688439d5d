"""A sliding window over a K/V cache against the plain causal call: tfa_fwd_kvcache_window (flash_attn_with_kvcache(sliding_window=w)) against the plain causal
entry point of the same library on the same cache, each at its own suggested split count — the plain call timed twice per round: its own repeat spread; never the
windowed call against itself.  H32 Hk8 D128 bf16 q, 256-key pages reached through a shuffled block table, 16384 keys per sequence.
  decode: Nq = 1, B in {1, 8, 64}, w in {1024, 4096}, a bf16 and an e4m3 cache (4-D form, tfa_fwd_kvcache_pack with TFA_PACK_GQA_AUTO as the baseline);
  mix:    60 decode rows + 4 chunks of 512 rows over 8192-key prefixes through cu_seqlens_q + scheduler_metadata, w = 1024 (tfa_fwd_kvcache_varlen_sched as the baseline).
Through the C ABI with prebuilt parameter blocks; times are HIP events around `iters` back-to-back calls (after warm-up calls), best of `--rounds` rounds, the arms
alternated in one process.
Expectation, written down before any measurement: the windowed call's time follows the K/V bytes of [lo64_b, len_b) — 1/16 (w = 1024) and 1/4 (w = 4096) of the
plain call's at B = 64, where the plain call is bandwidth-bound — and a floor of about two launches (30-35 us in the B = 1 rows of the other tables: the partial pass
and the merge) binds at small B, where the windowed call can be no faster than that floor whatever the window.
usage: python tools/bench_kvcache_window.py [--batches 1,8,64] [--windows 1024,4096] [--iters 10] [--rounds 3] [--out profiles/kvcache_window_bench.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib  # noqa: E402
from tools.bench_window import timeit  # noqa: E402

H, HK, D, PAGE, KEYS = 32, 8, 128, 256, 16384
SCALE = 1.0 / math.sqrt(D)
AUTO, ON = _lib.TFA_PACK_GQA_AUTO, _lib.TFA_PACK_GQA_ON


def pool(n_pages, fp8, dev):
    x = torch.empty((n_pages, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
    return x.to(torch.float8_e4m3fn) if fp8 else x


def cache_block(p, kc, vc, bt, lens_d, cap):
    p.k_cache, p.v_cache, p.cache_seqlens = kc.data_ptr(), vc.data_ptr(), lens_d.data_ptr()
    p.capacity = cap
    p.block_table, p.block_table_stride, p.page_size, p.num_pages = bt.data_ptr(), bt.stride(0), PAGE, kc.shape[0]
    for sname, t in (("k_stride", kc), ("v_stride", vc)):
        arr = getattr(p, sname)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.softmax_scale, p.is_causal, p.dtype = SCALE, 1, _lib.TFA_BF16


def race(arms, rounds, iters):
    best = [math.inf] * len(arms)
    for _ in range(rounds):
        for i, (_, f) in enumerate(arms):
            best[i] = min(best[i], timeit(f, iters))
    torch.cuda.synchronize()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--windows", default="1024,4096")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-mix", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# a sliding window over a K/V cache: H{H} Hk{HK} D{D} bf16 q, page {PAGE}, {KEYS} keys; tfa_fwd_kvcache_window vs the plain causal call (twice: its repeat")
    emit(f"# spread), each at its own suggested split count; HIP events, best of {a.rounds} rounds x {a.iters} calls, arms alternated.  GB/s: the K/V bytes of [lo64_b, len_b)")
    windows = [int(w) for w in a.windows.split(",")]
    for fp8 in (False, True):
        es = 1 if fp8 else 2
        for B in (int(b) for b in a.batches.split(",")):
            mb = KEYS // PAGE
            kc, vc = pool(B * mb, fp8, dev), pool(B * mb, fp8, dev)
            bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
            q = torch.empty((B, 1, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
            lens_d = torch.full((B,), KEYS, dtype=torch.int32, device=dev)
            outs = [torch.empty((B, H, 1, D), dtype=torch.bfloat16, device=dev) for _ in range(1 + len(windows))]
            lses = [torch.empty((B, H, 1), dtype=torch.float32, device=dev) for _ in range(1 + len(windows))]
            ps = []
            for o, l in zip(outs, lses):
                p = _lib.TfaKvcacheParams()
                p.q, p.out, p.lse = q.data_ptr(), o.data_ptr(), l.data_ptr()
                p.B, p.H, p.Hk, p.Nq, p.D = B, H, HK, 1, D
                p.q_stride[0], p.q_stride[1], p.q_stride[2] = H * D, D, H * D
                p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * D, D, D
                cache_block(p, kc, vc, bt, lens_d, KEYS)
                ps.append(p)
            p8 = _lib.TfaKvcacheFp8()
            p8.format = _lib.TFA_KV_E4M3
            q8 = C.byref(p8) if fp8 else None
            s0 = L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(ps[0]), AUTO)
            sw = [L.tfa_fwd_kvcache_window_suggest_splits(C.byref(p), None, AUTO, w - 1) for p, w in zip(ps[1:], windows)]
            need = max([L.tfa_fwd_kvcache_pack_workspace(C.byref(ps[0]), q8, AUTO, s0)]
                       + [L.tfa_fwd_kvcache_window_workspace(C.byref(p), None, q8, AUTO, w - 1, s) for p, w, s in zip(ps[1:], windows, sw)])
            if need < 0:
                _lib.check(int(need))
            ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
            plain = lambda: _lib.check(L.tfa_fwd_kvcache_pack(C.byref(ps[0]), q8, AUTO, s0, ws.data_ptr(), stream))      # noqa: E731
            arms = [(f"plain causal (splits {s0})", plain), ("plain causal, again", plain)]
            for p, w, s in zip(ps[1:], windows, sw):
                arms.append((f"sliding_window {w} (splits {s})",
                             lambda p=p, w=w, s=s: _lib.check(L.tfa_fwd_kvcache_window(C.byref(p), None, q8, AUTO, w - 1, s, None, ws.data_ptr(), stream))))
            best = race(arms, a.rounds, a.iters)
            emit(f"decode, {'e4m3' if fp8 else 'bf16'} cache, B {B}, Nq 1:")
            for i, ((label, _), ms) in enumerate(zip(arms, best)):
                keys = KEYS if i < 2 else KEYS - ((KEYS - 1 - (windows[i - 2] - 1)) & ~63)
                gb = 2.0 * B * HK * keys * D * es / 1e9
                emit(f"  {label:36s} {ms * 1e3:9.1f} us   {ms / best[0]:5.2f} x the plain call's time   {keys:6d} keys  {gb / (ms * 1e-3):8.1f} GB/s")
            del kc, vc
            torch.cuda.empty_cache()
    if not a.no_mix:
        nq, lens, cap, w = [1] * 60 + [512] * 4, [16384] * 60 + [8192 + 512] * 4, 16384, 1024
        B, total_q, max_q = len(nq), sum(nq), max(nq)
        mb = cap // PAGE
        kc, vc = pool(B * mb, False, dev), pool(B * mb, False, dev)
        bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
        q = torch.empty((total_q, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        cu = torch.tensor([0] + list(torch.tensor(nq).cumsum(0)), dtype=torch.int32, device=dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        outs = [torch.empty((H, total_q, D), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        lses = [torch.empty((H, total_q), dtype=torch.float32, device=dev) for _ in range(2)]
        ps = []
        for o, l in zip(outs, lses):
            p = _lib.TfaKvcacheParams()
            p.q, p.out, p.lse = q.data_ptr(), o.data_ptr(), l.data_ptr()
            p.B, p.H, p.Hk, p.D = B, H, HK, D
            p.q_stride[1], p.q_stride[2] = q.stride(1), q.stride(0)
            p.o_stride[1], p.o_stride[2] = total_q * D, D
            cache_block(p, kc, vc, bt, lens_d, cap)
            ps.append(p)
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, total_q
        s0 = L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(ps[0]), C.byref(vq), ON)
        s1 = L.tfa_fwd_kvcache_window_suggest_splits(C.byref(ps[1]), C.byref(vq), ON, w - 1)
        need = max(L.tfa_fwd_kvcache_varlen_workspace(C.byref(ps[0]), C.byref(vq), None, ON, s0),
                   L.tfa_fwd_kvcache_window_workspace(C.byref(ps[1]), C.byref(vq), None, ON, w - 1, s1))
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
        size = L.tfa_kvcache_varlen_schedule_size(C.byref(ps[0]), C.byref(vq), ON, 1)
        if size < 0:
            _lib.check(int(size))
        meta = torch.zeros((int(size),), dtype=torch.int32, device=dev)
        _lib.check(L.tfa_kvcache_varlen_schedule(C.byref(ps[0]), C.byref(vq), ON, 1, C.c_void_p(meta.data_ptr()), stream))
        torch.cuda.synchronize()
        mp = C.c_void_p(meta.data_ptr())
        plain = lambda: _lib.check(L.tfa_fwd_kvcache_varlen_sched(C.byref(ps[0]), C.byref(vq), None, ON, s0, mp, ws.data_ptr(), stream))      # noqa: E731
        win = lambda: _lib.check(L.tfa_fwd_kvcache_window(C.byref(ps[1]), C.byref(vq), None, ON, w - 1, s1, mp, ws.data_ptr(), stream))      # noqa: E731
        arms = [(f"plain causal, scheduled (splits {s0})", plain), ("plain causal, scheduled, again", plain), (f"sliding_window {w}, scheduled (splits {s1})", win)]
        best = race(arms, a.rounds, a.iters)
        kb = [sum(lens), sum(lens), sum(n - (max(0, n - m - (w - 1)) & ~63) for n, m in zip(lens, nq))]
        emit(f"mix: 60 decode rows (16384 keys) + 4 chunks of 512 rows over 8192-key prefixes, bf16 cache, cu_seqlens_q + scheduler_metadata, B {B}, total_q {total_q}:")
        for (label, _), ms, keys in zip(arms, best, kb):
            gb = 2.0 * HK * keys * D * 2 / 1e9
            emit(f"  {label:44s} {ms * 1e3:9.1f} us   {ms / best[0]:5.2f} x the plain call's time   {keys:7d} keys  {gb / (ms * 1e-3):8.1f} GB/s")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
