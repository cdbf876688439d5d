"""Shared-prefix (cascade) attention against the flat packed-q call of the same library: tfa_fwd_kvcache_cascade (the shared pages once per group, each sequence's own
pages once, one merge) vs tfa_fwd_kvcache_varlen over full per-sequence tables with the shared pages repeated in every row (timed twice per round: its repeat
spread).  H32 Hk8 D128 bf16, causal, 256-key pages through shuffled tables.  64 decode rows in groups of {1, 4, 16, 64} over an 8192-key shared prefix plus 256 own
keys; and one mix with a 512-row prefill chunk (a group of its own, over its own 8192-key prefix) beside 63 decode rows in groups of 16 (the last of 15).  Each arm
runs at its own suggested split counts.  Through the C ABI with prebuilt parameter blocks; times are HIP events around `iters` back-to-back calls (after warm-up
calls), best of `--rounds` rounds, the arms alternated in one process.
Expectation, written down before any measurement: the K/V bytes fall from 64 x 8448 keys to Gn x 8192 + 64 x 256, so groups of 16 and 64 should win by a large
factor; the call is four launches (a fill, two passes, a merge), so the 30-35 us floor of small calls binds first and groups of 1 — same bytes, more launches, a
merge the flat call may not need — should lose to the flat call.
usage: python tools/bench_kvcache_cascade.py [--iters 10] [--rounds 3] [--out profiles/kvcache_cascade_bench.txt]"""
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

H, HK, D, PAGE = 32, 8, 128, 256
SCALE = 1.0 / math.sqrt(D)
PLEN, ULEN = 8192, 256
MIXES = [(f"64 decode rows in groups of {g}", [1] * 64, [g] * (64 // g)) for g in (1, 4, 16, 64)]
MIXES.append(("a 512-row prefill chunk + 63 decode rows in groups of 16", [512] + [1] * 63, [1, 16, 16, 16, 15]))


def params(q, dense, lse, kc, vc, lens, bt, cap, B):
    p = _lib.TfaKvcacheParams()
    p.q, p.out, p.lse, p.k_cache, p.v_cache, p.cache_seqlens = q.data_ptr(), dense.data_ptr(), lse.data_ptr(), kc.data_ptr(), vc.data_ptr(), lens.data_ptr()
    p.B, p.H, p.Hk, p.D, p.capacity = B, H, HK, D, cap
    p.block_table, p.block_table_stride, p.page_size, p.num_pages = bt.data_ptr(), bt.stride(0), PAGE, kc.shape[0]
    p.q_stride[1], p.q_stride[2] = q.stride(1), q.stride(0)
    p.o_stride[1], p.o_stride[2] = q.shape[0] * D, D
    for sname, t in (("k_stride", kc), ("v_stride", vc)):
        arr = getattr(p, sname)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.softmax_scale, p.is_causal, p.dtype = SCALE, 1, _lib.TFA_BF16
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ON = _lib.TFA_PACK_GQA_ON
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# shared-prefix attention over a paged K/V cache: H{H} Hk{HK} D{D} bf16 causal, page {PAGE}, {PLEN} shared + own keys per sequence ({ULEN} behind a decode row);")
    emit(f"# tfa_fwd_kvcache_cascade vs tfa_fwd_kvcache_varlen over full tables (twice); each at its suggested splits; HIP events, best of {a.rounds} rounds x {a.iters} calls, arms alternated")
    for what, nq, sizes in MIXES:
        B, Gn, total_q, max_q = len(nq), len(sizes), sum(nq), max(nq)
        own = [ULEN if n == 1 else n for n in nq]                       # own keys, this step's rows included
        mb, pmb = (max(own) + PAGE - 1) // PAGE, PLEN // PAGE
        npages = B * mb + Gn * pmb
        gen = torch.Generator().manual_seed(99)
        kc = torch.empty((npages, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vc = torch.empty((npages, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        perm = torch.randperm(npages, generator=gen).to(torch.int32)
        bt_h, pbt_h = perm[:B * mb].view(B, mb), perm[B * mb:].view(Gn, pmb)
        grp = [g for g, n in enumerate(sizes) for _ in range(n)]
        flat_h = torch.cat([torch.stack([pbt_h[g] for g in grp]), bt_h], dim=1).contiguous()       # the shared pages repeated in every sequence's row
        q = torch.empty((total_q, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        cu_h = torch.tensor([0] + list(torch.tensor(nq).cumsum(0)), dtype=torch.int32)
        ends = torch.tensor(sizes).cumsum(0)
        pcu_h = torch.cat([cu_h[:1], cu_h[ends]])
        pmax_q = int((pcu_h[1:] - pcu_h[:-1]).max())
        cu, pcu, bt, pbt, flat_bt = (x.to(dev) for x in (cu_h, pcu_h, bt_h.contiguous(), pbt_h.contiguous(), flat_h))
        lens = torch.tensor(own, dtype=torch.int32, device=dev)
        plens = torch.full((Gn,), PLEN, dtype=torch.int32, device=dev)
        flens = lens + PLEN
        outs, arms = [], []

        # this call
        dense, lse = torch.empty((H, total_q, D), dtype=torch.bfloat16, device=dev), torch.empty((H, total_q), dtype=torch.float32, device=dev)
        p = params(q, dense, lse, kc, vc, lens, bt, mb * PAGE, B)
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, total_q
        cs = _lib.TfaKvcacheCascade()
        cs.prefix_cu_seqlens_q, cs.prefix_seqlens, cs.prefix_block_table = pcu.data_ptr(), plens.data_ptr(), pbt.data_ptr()
        cs.prefix_block_table_stride, cs.num_groups, cs.prefix_max_blocks, cs.prefix_max_seqlen_q = pbt.stride(0), Gn, pmb, pmax_q
        s1, s0 = C.c_int(), C.c_int()
        _lib.check(L.tfa_fwd_kvcache_cascade_suggest_splits(C.byref(p), C.byref(vq), C.byref(cs), ON, C.byref(s1), C.byref(s0)))
        s1, s0 = max(1, s1.value), max(1, s0.value)
        need = L.tfa_fwd_kvcache_cascade_workspace(C.byref(p), C.byref(vq), C.byref(cs), ON, s1, s0)
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty((int(need),), dtype=torch.float32, device=dev)
        g0, g1 = C.c_int(), C.c_int()
        _lib.check(L.tfa_fwd_kvcache_cascade_plan(C.byref(p), C.byref(vq), C.byref(cs), ON, s1, s0, 0, 0, 0, C.byref(g0), None, None))
        _lib.check(L.tfa_fwd_kvcache_cascade_plan(C.byref(p), C.byref(vq), C.byref(cs), ON, s1, s0, 0, 0, 1, C.byref(g1), None, None))
        arms.append((f"cascade (splits {s0} + {s1}, grids {g0.value} + {g1.value})",
                     lambda: _lib.check(L.tfa_fwd_kvcache_cascade(C.byref(p), C.byref(vq), C.byref(cs), ON, s1, s0, None, None, ws.data_ptr(), stream))))

        # the flat call over full tables
        dense2, lse2 = torch.empty_like(dense), torch.empty_like(lse)
        pf = params(q, dense2, lse2, kc, vc, flens, flat_bt, (pmb + mb) * PAGE, B)
        sf = max(1, L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(pf), C.byref(vq), ON))
        needf = L.tfa_fwd_kvcache_varlen_workspace(C.byref(pf), C.byref(vq), None, ON, sf)
        if needf < 0:
            _lib.check(int(needf))
        wsf = torch.empty((max(int(needf), 4),), dtype=torch.float32, device=dev)
        gf = C.c_int()
        _lib.check(L.tfa_fwd_kvcache_varlen_plan(C.byref(pf), C.byref(vq), None, ON, sf, C.byref(gf), None, None))
        flat = lambda: _lib.check(L.tfa_fwd_kvcache_varlen(C.byref(pf), C.byref(vq), None, ON, sf, wsf.data_ptr(), stream))      # noqa: E731
        arms.append((f"flat packed-q (splits {sf}, grid {gf.value})", flat))
        arms.append(("flat packed-q, again", flat))

        best = [math.inf] * len(arms)
        for _ in range(a.rounds):
            for i, (_, f) in enumerate(arms):
                best[i] = min(best[i], timeit(f, a.iters))
        torch.cuda.synchronize()
        d = (dense.float() - dense2.float()).abs().max().item()
        b_casc = 2.0 * (Gn * PLEN + sum(own)) * HK * D * 2
        b_flat = 2.0 * (B * PLEN + sum(own)) * HK * D * 2
        emit(f"{what}: B {B}, groups {Gn}, total_q {total_q}; K/V bytes {b_casc / 1e6:.1f} MB vs {b_flat / 1e6:.1f} MB flat; max|out - flat out| = {d:.2e}")
        for (label, _), ms, nbytes in zip(arms, best, (b_casc, b_flat, b_flat)):
            emit(f"  {label:52s} {ms * 1e3:9.1f} us   {nbytes / (ms * 1e-3) / 1e12:6.2f} TB/s of the arm's own K/V bytes   {ms / best[0]:5.2f} x the cascade call's time")
        del arms, kc, vc, outs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
