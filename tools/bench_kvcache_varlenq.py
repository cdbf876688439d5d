"""Packed ragged query rows over a paged K/V cache: tfa_fwd_kvcache_varlen (flash_attn_with_kvcache(cu_seqlens_q=): the varlen-q form of the KV-cache kernel,
GQA rows packed, at its own suggested split count) against tfa_fwd_varlen_paged on the same batch (flash_attn_varlen_func(block_table=): the il kernels, the route
a unified batch took before) and, for the pure-decode mix, against tfa_fwd_kvcache_pack(ON) with Nq = 1 (the 4-D call, timed twice per round: its repeat spread).
H32 Hk8 D128 bf16, causal, 256-key pages reached through a shuffled block table.  Mixes: (a) pure decode, 64 sequences of 16384 keys, one row each; (b) 60 such
decode rows + 4 chunks of 512 rows over 8192-key prefixes; (c) pure prefill, 4 x 2048 rows.  Through the C ABI with prebuilt parameter blocks; times are HIP
events around `iters` back-to-back calls (after warm-up calls), best of `--rounds` rounds, the arms alternated in one process.
Expectation, written down before any measurement: on (a) parity with the 4-D call within that arm's own repeat spread, and several times ahead of the paged-varlen
route (K / V bytes are G = 4 times fewer, and a decode row no longer occupies a 128- / 256-row query block per head); on (c) the il kernels are expected to win
(hand-scheduled tile loops, 256-row blocks; here the grid is sized by max_seqlen_q and every block streams its keys through the two-buffer LDS-DMA loop).
usage: python tools/bench_kvcache_varlenq.py [--mixes a,b,c] [--iters 10] [--rounds 3] [--out profiles/kvcache_varlenq_bench.txt]"""
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
MIXES = {                      # name: (rows per sequence, keys per sequence INCLUDING this step's rows, capacity)
    "a": ("pure decode: 64 x 1 row over 16384 keys", [1] * 64, [16384] * 64, 16384),
    "b": ("60 decode rows (16384 keys) + 4 chunks of 512 rows over 8192-key prefixes", [1] * 60 + [512] * 4, [16384] * 60 + [8192 + 512] * 4, 16384),
    "c": ("pure prefill: 4 x 2048 rows", [2048] * 4, [2048] * 4, 2048),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixes", default="a,b,c")
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

    emit(f"# packed ragged query rows over a paged K/V cache: H{H} Hk{HK} D{D} bf16 causal, page {PAGE}; tfa_fwd_kvcache_varlen (packed, its suggested splits) vs")
    emit(f"# tfa_fwd_varlen_paged on the same batch vs (mix a) tfa_fwd_kvcache_pack(ON) at Nq = 1; HIP events, best of {a.rounds} rounds x {a.iters} calls, arms alternated")
    for name in a.mixes.split(","):
        what, nq, lens, cap = MIXES[name]
        B, total_q, max_q = len(nq), sum(nq), max(nq)
        mb = cap // PAGE
        kc = torch.empty((B * mb, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vc = torch.empty((B * mb, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
        q = torch.empty((total_q, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        cu = torch.tensor([0] + list(torch.tensor(nq).cumsum(0)), dtype=torch.int32, device=dev)
        cu_k = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        keep, arms = [], []

        # this call
        dense = torch.empty((H, total_q, D), dtype=torch.bfloat16, device=dev)
        lse = torch.empty((H, total_q), dtype=torch.float32, device=dev)
        p = _lib.TfaKvcacheParams()
        p.q, p.out, p.lse, p.k_cache, p.v_cache, p.cache_seqlens = q.data_ptr(), dense.data_ptr(), lse.data_ptr(), kc.data_ptr(), vc.data_ptr(), lens_d.data_ptr()
        p.B, p.H, p.Hk, p.D, p.capacity = B, H, HK, D, cap
        p.block_table, p.block_table_stride, p.page_size, p.num_pages = bt.data_ptr(), bt.stride(0), PAGE, B * mb
        p.q_stride[1], p.q_stride[2] = q.stride(1), q.stride(0)
        p.o_stride[1], p.o_stride[2] = total_q * D, D
        for sname, t in (("k_stride", kc), ("v_stride", vc)):
            arr = getattr(p, sname)
            arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
        p.softmax_scale, p.is_causal, p.dtype = SCALE, 1, _lib.TFA_BF16
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, total_q
        s_vq = L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(p), C.byref(vq), _lib.TFA_PACK_GQA_ON)
        need = L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, _lib.TFA_PACK_GQA_ON, s_vq)
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
        g = C.c_int()
        _lib.check(L.tfa_fwd_kvcache_varlen_plan(C.byref(p), C.byref(vq), None, _lib.TFA_PACK_GQA_ON, s_vq, C.byref(g), None, None))
        arms.append((f"kvcache varlen-q (splits {s_vq}, grid {g.value})",
                     lambda: _lib.check(L.tfa_fwd_kvcache_varlen(C.byref(p), C.byref(vq), None, _lib.TFA_PACK_GQA_ON, s_vq, ws.data_ptr(), stream))))

        # today's route for the same batch
        out2 = torch.empty_like(q)
        lse2 = torch.empty((H, total_q), dtype=torch.float32, device=dev)
        pv = _lib.TfaVarlenFwdParams()
        pv.q, pv.k, pv.v, pv.out, pv.lse = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out2.data_ptr(), lse2.data_ptr()
        pv.cu_seqlens_q, pv.cu_seqlens_k = cu.data_ptr(), cu_k.data_ptr()
        pv.B, pv.H, pv.Hk, pv.D = B, H, HK, D
        pv.max_seqlen_q, pv.max_seqlen_k, pv.total_q, pv.total_k = max_q, max(lens), total_q, 0
        for sname, t in (("q_stride", q), ("o_stride", out2)):
            arr = getattr(pv, sname)
            arr[0], arr[1] = t.stride(1), t.stride(0)
        for sname, t in (("k_stride", kc), ("v_stride", vc)):
            arr = getattr(pv, sname)
            arr[0], arr[1] = t.stride(2), t.stride(1)
        pv.softmax_scale, pv.is_causal, pv.dtype, pv.out_dtype = SCALE, 1, _lib.TFA_BF16, _lib.TFA_BF16
        pg = _lib.TfaPagedKv()
        pg.block_table, pg.table_stride, pg.max_blocks = bt.data_ptr(), bt.stride(0), mb
        pg.page_size, pg.num_pages, pg.k_page_stride, pg.v_page_stride = PAGE, B * mb, kc.stride(0), vc.stride(0)
        arms.append(("varlen paged (il kernels)", lambda: _lib.check(L.tfa_fwd_varlen_paged(C.byref(pv), C.byref(pg), stream))))

        if max_q == 1:         # the 4-D call on the same rows, twice: its repeat spread
            q4 = q.view(B, 1, H, D)
            out4 = torch.empty((B, H, 1, D), dtype=torch.bfloat16, device=dev)
            lse4 = torch.empty((B, H, 1), dtype=torch.float32, device=dev)
            p4 = ops._kvcache_params(q4, kc, vc, out4, lse4, lens_d, bt, None, None, SCALE, True)
            s4 = L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(p4), _lib.TFA_PACK_GQA_ON)
            need4 = L.tfa_fwd_kvcache_pack_workspace(C.byref(p4), None, _lib.TFA_PACK_GQA_ON, s4)
            ws4 = torch.empty((max(int(need4), 4),), dtype=torch.float32, device=dev)
            f4 = lambda: _lib.check(L.tfa_fwd_kvcache_pack(C.byref(p4), None, _lib.TFA_PACK_GQA_ON, s4, ws4.data_ptr(), stream))
            arms.append((f"kvcache 4-D pack ON Nq 1 (splits {s4})", f4))
            arms.append(("kvcache 4-D pack ON Nq 1, again", f4))
            keep += [q4, out4, lse4, ws4]

        best = [math.inf] * len(arms)
        for _ in range(a.rounds):
            for i, (_, f) in enumerate(arms):
                best[i] = min(best[i], timeit(f, a.iters))
        torch.cuda.synchronize()
        d = (dense.transpose(0, 1).float() - out2.float()).abs().max().item()
        kv_bytes = 2.0 * sum(lens) * HK * D * 2
        emit(f"mix ({name}) {what}: B {B}, total_q {total_q}, max_seqlen_q {max_q}; max|out - paged varlen out| = {d:.2e}")
        for (label, _), ms in zip(arms, best):
            emit(f"  {label:48s} {ms:9.4f} ms   {kv_bytes / (ms * 1e-3) / 1e12:6.2f} TB/s of K/V counted once   {ms / best[0]:5.2f} x this call's time")
        del keep, arms, kc, vc
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
