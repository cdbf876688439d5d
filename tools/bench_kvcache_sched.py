"""The scheduled packed-q K/V-cache call against the unscheduled one: tfa_fwd_kvcache_varlen_sched with a prebuilt work list (tfa_kvcache_varlen_schedule;
get_scheduler_metadata / scheduler_metadata= in Python) against tfa_fwd_kvcache_varlen of the same library on the same batch, at the same (suggested) split count —
the unscheduled call timed twice per round: its own repeat spread — and the schedule launch alone.  H32 Hk8 D128 bf16, causal, GQA rows packed, 256-key pages
reached through a shuffled block table.  Mixes: (a) pure decode, 64 sequences of 16384 keys, one row each; (b) 60 such decode rows + 4 chunks of 512 rows over
8192-key prefixes; (d) skewed: 255 decode rows over 8192 keys + one 2048-row chunk over an 8192-key prefix.  Through the C ABI with prebuilt parameter blocks;
times are HIP events around `iters` back-to-back calls (after warm-up calls), best of `--rounds` rounds, the arms alternated in one process.
Expectation, written down before any measurement: on (a) the scheduled call within the unscheduled arm's own repeat spread plus whatever one more scalar load per
item costs (the two grids are the same size); on (d) clearly ahead (the unscheduled launch carries ~130 000 workgroups per chunk, about a thousand hold a row); on
(b) a little ahead; the schedule launch a few microseconds, paid once per step, not per layer.
usage: python tools/bench_kvcache_sched.py [--mixes a,b,d] [--iters 10] [--rounds 3] [--out profiles/kvcache_sched_bench.txt]"""
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
ON = _lib.TFA_PACK_GQA_ON
MIXES = {                      # name: (rows per sequence, keys per sequence INCLUDING this step's rows, capacity)
    "a": ("pure decode: 64 x 1 row over 16384 keys", [1] * 64, [16384] * 64, 16384),
    "b": ("60 decode rows (16384 keys) + 4 chunks of 512 rows over 8192-key prefixes", [1] * 60 + [512] * 4, [16384] * 60 + [8192 + 512] * 4, 16384),
    "d": ("skewed: 255 decode rows (8192 keys) + one chunk of 2048 rows over an 8192-key prefix", [1] * 255 + [2048], [8192] * 255 + [8192 + 2048], 8192 + 2048),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixes", default="a,b,d")
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

    emit(f"# the scheduled packed-q K/V-cache call: H{H} Hk{HK} D{D} bf16 causal, GQA rows packed, page {PAGE}; tfa_fwd_kvcache_varlen_sched (prebuilt list) vs")
    emit(f"# tfa_fwd_kvcache_varlen (twice: its repeat spread) at the same split count, and tfa_kvcache_varlen_schedule alone; HIP events, best of {a.rounds} rounds x "
         f"{a.iters} calls, arms alternated")
    for name in a.mixes.split(","):
        what, nq, lens, cap = MIXES[name]
        B, total_q, max_q = len(nq), sum(nq), max(nq)
        mb = cap // PAGE
        kc = torch.empty((B * mb, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        vc = torch.empty((B * mb, PAGE, HK, D), dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
        q = torch.empty((total_q, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
        cu = torch.tensor([0] + list(torch.tensor(nq).cumsum(0)), dtype=torch.int32, device=dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)

        def block(dense, lse):
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
            return p

        out_u, lse_u = torch.empty((H, total_q, D), dtype=torch.bfloat16, device=dev), torch.empty((H, total_q), dtype=torch.float32, device=dev)
        out_s, lse_s = torch.empty_like(out_u), torch.empty_like(lse_u)
        pu, ps = block(out_u, lse_u), block(out_s, lse_s)
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, total_q
        splits = L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(pu), C.byref(vq), ON)
        need = L.tfa_fwd_kvcache_varlen_workspace(C.byref(pu), C.byref(vq), None, ON, splits)
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
        size = L.tfa_kvcache_varlen_schedule_size(C.byref(ps), C.byref(vq), ON, 1)
        if size < 0:
            _lib.check(int(size))
        meta = torch.zeros((int(size),), dtype=torch.int32, device=dev)
        build = lambda: _lib.check(L.tfa_kvcache_varlen_schedule(C.byref(ps), C.byref(vq), ON, 1, C.c_void_p(meta.data_ptr()), stream))
        build()
        torch.cuda.synchronize()
        n_items, bound = int(meta[0]), int(meta[6])
        gu, gs = C.c_int(), C.c_int()
        _lib.check(L.tfa_fwd_kvcache_varlen_plan(C.byref(pu), C.byref(vq), None, ON, splits, C.byref(gu), None, None))
        _lib.check(L.tfa_fwd_kvcache_varlen_sched_plan(C.byref(ps), C.byref(vq), None, ON, splits, C.byref(gs), None, None))
        unsched = lambda: _lib.check(L.tfa_fwd_kvcache_varlen(C.byref(pu), C.byref(vq), None, ON, splits, ws.data_ptr(), stream))
        sched = lambda: _lib.check(L.tfa_fwd_kvcache_varlen_sched(C.byref(ps), C.byref(vq), None, ON, splits, C.c_void_p(meta.data_ptr()), ws.data_ptr(), stream))
        arms = [(f"unscheduled (splits {splits}, grid {gu.value})", unsched), ("unscheduled, again", unsched),
                (f"scheduled (splits {splits}, grid {gs.value})", sched), ("the schedule launch alone", build)]
        best = [math.inf] * len(arms)
        for _ in range(a.rounds):
            for i, (_, f) in enumerate(arms):
                best[i] = min(best[i], timeit(f, a.iters))
        torch.cuda.synchronize()
        same = torch.equal(out_u, out_s) and torch.equal(lse_u, lse_s)
        emit(f"mix ({name}) {what}: B {B}, total_q {total_q}, max_seqlen_q {max_q}; list: {n_items} items, bound {bound}; out / lse bit-identical: {same}")
        for (label, _), ms in zip(arms, best):
            emit(f"  {label:48s} {ms * 1e3:10.1f} us   {ms / best[0]:5.2f} x the unscheduled call's time")
        del kc, vc
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
