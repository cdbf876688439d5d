"""Paged K/V in the packed variable-length forward (tfa_fwd_varlen_paged) against its ceiling and against what a caller had to do without it, in one
process, alternating.  H32 Hk8 D128 bf16 causal; three mixes:
  equal    4 x 4096 new tokens over themselves (the headline's shape as a packed batch)
  pack     the packing mix of tools/bench_varlen.py (documents of 512..8192 tokens filling four rows of 16k)
  chunked  chunked prefill: 8 sequences x 512 new tokens over prefixes of 4k..32k already in the pool
and four rows per mix:
  paged256    tfa_fwd_varlen_paged, pages of 256 keys, a shuffled block table
  paged64     the same with pages of 64 keys (one page per key tile: a table entry per tile)
  contiguous  tfa_fwd_varlen on the same keys already contiguous — the ceiling
  gather+call the pages gathered into a contiguous (total_k, Hk, D) buffer with torch.index_select (K and V; the row index is prebuilt, not timed), then
              tfa_fwd_varlen: what a caller must do without the paged form
The kernel calls go through the C ABI with prebuilt parameter blocks; times are HIP events around `iters` back-to-back calls after warm-up calls, best of
`--rounds` alternating rounds (the protocol of tools/bench_varlen.py).  TFLOP/s counts algorithmic flops: 4 * visible (query, key) pairs * D * H.
usage: python tools/bench_varlen_paged.py [--mixes equal,pack,chunked] [--iters 10] [--rounds 3] [--out profiles/varlen_paged_bench.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_varlen import mix_lengths, ops_varlen_params, timeit, visible_pairs  # noqa: E402
from tiny_flash_attention_amd import _lib  # noqa: E402


def mix_of(name):
    """(new tokens, keys) per sequence"""
    if name == "chunked":
        return [(512, 4096 * (b + 1) + 512) for b in range(8)]       # prefixes 4k, 8k, .., 32k + the 512 new tokens themselves
    return [(n, n) for n in mix_lengths(name)]


def pool_of(k, lk, page, dev, seed):
    """the contiguous keys k (total_k, Hk, D) laid out in a pool of `page`-key pages under a shuffled table: (pool, block_table, row index of key j in the pool)"""
    need = [(n + page - 1) // page for n in lk]
    num_pages = sum(need) + 8
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))
    bt = torch.zeros((len(lk), max(need)), dtype=torch.int32)
    pool = torch.zeros((num_pages, page) + tuple(k.shape[1:]), dtype=k.dtype, device=dev)
    rows, nxt, k0 = [], 0, 0
    for b, n in enumerate(lk):
        pages = perm[nxt:nxt + need[b]]
        nxt += need[b]
        bt[b, :need[b]] = pages.to(torch.int32)
        j = torch.arange(n)
        rows.append(pages[j // page] * page + j % page)
        k0 += n
    rows = torch.cat(rows).to(dev)
    pool.view(-1, *k.shape[1:]).index_copy_(0, rows, k)
    return pool, bt.to(dev), rows


def paged_params(p_contig, kp, vp, bt):
    p = _lib.TfaVarlenFwdParams.from_buffer_copy(p_contig)
    p.k, p.v, p.total_k = kp.data_ptr(), vp.data_ptr(), 0
    p.k_stride[0], p.k_stride[1] = kp.stride(2), kp.stride(1)
    p.v_stride[0], p.v_stride[1] = vp.stride(2), vp.stride(1)
    pg = _lib.TfaPagedKv()
    pg.block_table, pg.table_stride, pg.max_blocks = bt.data_ptr(), bt.stride(0), bt.shape[1]
    pg.page_size, pg.num_pages = kp.shape[1], kp.shape[0]
    pg.k_page_stride, pg.v_page_stride = kp.stride(0), vp.stride(0)
    return p, pg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixes", default="equal,pack,chunked")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_paged_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    dt, causal, H, Hk, D = torch.bfloat16, True, 32, 8, 128
    sc = 1.0 / math.sqrt(D)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["# tools/bench_varlen_paged.py: H32 Hk8 D128 bf16 causal; HIP events, best of %d rounds x %d calls; TFLOP/s = algorithmic flops" % (a.rounds, a.iters),
             "# paged256 / paged64: tfa_fwd_varlen_paged; contiguous: tfa_fwd_varlen on the same keys (the ceiling); gather+call: index_select of K and V + tfa_fwd_varlen"]
    for mix in a.mixes.split(","):
        seqs = mix_of(mix)
        lq, lk = [s[0] for s in seqs], [s[1] for s in seqs]
        cq = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32, device=dev)
        ck = torch.tensor([0] + list(torch.tensor(lk).cumsum(0)), dtype=torch.int32, device=dev)
        fl = 4.0 * H * D * sum(visible_pairs(nq, nk, causal) for nq, nk in seqs)
        mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev).normal_(0, 0.5).to(dt)
        q, k, v = mk(sum(lq), H, D), mk(sum(lk), Hk, D), mk(sum(lk), Hk, D)
        out = torch.empty_like(q)
        lse = torch.empty((H, sum(lq)), dtype=torch.float32, device=dev)
        pc = ops_varlen_params(q, k, v, out, lse, cq, max(lq), causal, sc)
        pc.cu_seqlens_k, pc.max_seqlen_k = ck.data_ptr(), max(lk)
        arms, keep = {}, []
        for page in (256, 64):
            kp, bt, rows = pool_of(k, lk, page, dev, seed=page)
            vp, _, _ = pool_of(v, lk, page, dev, seed=page)
            pp, pg = paged_params(pc, kp, vp, bt)
            keep.append((kp, vp, bt, rows, pp, pg))
            arms[f"paged{page}"] = (lambda pp=pp, pg=pg: _lib.check(L.tfa_fwd_varlen_paged(C.byref(pp), C.byref(pg), st)))
        arms["contiguous"] = lambda: _lib.check(L.tfa_fwd_varlen(C.byref(pc), st))
        kp, vp, _, rows, _, _ = keep[0]
        kg, vg = torch.empty_like(k), torch.empty_like(v)
        pgc = ops_varlen_params(q, kg, vg, out, lse, cq, max(lq), causal, sc)
        pgc.cu_seqlens_k, pgc.max_seqlen_k = ck.data_ptr(), max(lk)

        def gather_call():
            torch.index_select(kp.view(-1, Hk, D), 0, rows, out=kg)
            torch.index_select(vp.view(-1, Hk, D), 0, rows, out=vg)
            _lib.check(L.tfa_fwd_varlen(C.byref(pgc), st))

        arms["gather+call"] = gather_call
        # the arms agree before they are timed (paged against contiguous: same keys)
        ref = torch.empty_like(out)
        arms["contiguous"]()
        ref.copy_(out)
        for n in ("paged256", "paged64", "gather+call"):
            arms[n]()
            torch.cuda.synchronize()
            assert (out.float() - ref.float()).abs().max().item() <= 2e-2, n
        best = {n: float("inf") for n in arms}
        for _ in range(a.rounds):
            for n, fn in arms.items():
                best[n] = min(best[n], timeit(fn, a.iters))
        var = L.tfa_fwd_varlen_paged_variant(C.byref(keep[0][4]), C.byref(keep[0][5]))
        lines.append(f"{mix:8s} B{len(seqs):<3d} new tokens {sum(lq):6d} keys {sum(lk):7d} (max {max(lq)} x {max(lk)}) variant {var}")
        for n, ms in best.items():
            lines.append(f"    {n:12s} {ms:8.3f} ms {fl / ms / 1e9:7.1f} TF   {best['contiguous'] / ms:5.3f} of contiguous")
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
