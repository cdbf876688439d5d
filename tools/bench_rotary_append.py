"""The serving step's parts around attention: tfa_rotary and tfa_kvcache_append_varlen through the C ABI with prebuilt parameter blocks, against the same work done
by a torch composition (rotate-half with elementwise ops; slot indices with index_put_), the two alternated in one process.  HIP events around `iters` back-to-back
calls, best of `--rounds` rounds.  GB/s counts the bytes each shape has to move: rotary = read + write of the rotated tensors (in place: the same count, the rows
are read and written once) plus the table rows; append = read of k / v plus write of the slots (plus the table rows with fused RoPE).
  rotary:  q + k at 4 x 4096, H32 / Hk8, D128 = rotary_dim, bf16, both layouts, in place and out of place (one launch for both tensors)
  append:  the "56 short + 4 long" prefill mix of tools/bench_varlen.py (Hk8, D128, bf16) into 256-key pages through a shuffled table, with and without fused RoPE
  decode:  B = 64, one row per sequence — rotary of q + k, and the packed append of 64 rows (launch-latency bound)
  ex:      tfa_kvcache_append_varlen_ex at the same two append shapes — the append into an e4m3 pool, plain and with fused RoPE, alternated with the 16-bit
           append of the same rows; and the append with q rotated in its launch (16-bit pool, H32 q), alternated with what the step needs without it:
           tfa_kvcache_append_varlen with tables plus tfa_rotary on q in place (two launches)
Expectation before measuring: the large shapes are bound by HBM bytes, the decode shapes by launch latency; the fp8 append moves three quarters of the 16-bit
append's bytes; the fused-q call saves about one launch at decode shapes.
usage: python tools/bench_rotary_append.py [--iters 10] [--rounds 3] [--out profiles/rotary_append_bench.txt] [--ex-out profiles/append_varlen_ex_bench.txt] [--only-ex]"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_flash_attention_amd import _lib, ops  # noqa: E402
from tools.bench_varlen import mix_lengths  # noqa: E402
from tools.bench_window import timeit  # noqa: E402

H, HK, D, PAGE, RO = 32, 8, 128, 256, 16384
DT = torch.bfloat16


def torch_rotary(x, cos, sin, pos, interleaved):
    """The torch composition: x (R, h, D) rotated at pos (R,), fp32 arithmetic, elementwise ops."""
    c, s = cos[pos][:, None, :].float(), sin[pos][:, None, :].float()
    xf = x.float()
    if interleaved:
        x1, x2 = xf[..., 0::2], xf[..., 1::2]
        return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), -1).flatten(-2).to(x.dtype)
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    return torch.cat((x1 * c - x2 * s, x1 * s + x2 * c), -1).to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ex-out", default=None, help="file for the tfa_kvcache_append_varlen_ex rows")
    ap.add_argument("--only-ex", action="store_true", help="skip the rotary and plain-append rows")
    a = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    ex_lines = []

    def emit(s, to=None):
        print(s, flush=True)
        (lines if to is None else to).append(s)

    def race(tfa_call, torch_call):
        best = [math.inf, math.inf]
        for _ in range(a.rounds):
            for i, f in enumerate((tfa_call, torch_call)):
                best[i] = min(best[i], timeit(f, a.iters))
        return best

    ang = torch.arange(RO, dtype=torch.float64)[:, None] / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))[None, :]
    cos, sin = ang.cos().to(DT).to(dev), ang.sin().to(DT).to(dev)
    emit(f"# rotary embedding and packed K/V append, H{H} Hk{HK} D{D} rotary_dim {D} bf16, page {PAGE}; HIP events, best of {a.rounds} rounds x {a.iters} calls")
    emit("# tfa = one C-ABI call (tfa_rotary / tfa_kvcache_append_varlen); torch = the same work as elementwise ops / index_put_; GB/s over the bytes the shape must move")
    emit(f"# {'shape':<58} | {'tfa ms':>8} {'GB/s':>7} | {'torch ms':>8} {'GB/s':>7} | {'torch / tfa':>11}")

    def row(label, nbytes, t):
        emit(f"  {label:<58} | {t[0]:8.4f} {nbytes / (t[0] * 1e-3) / 1e9:7.0f} | {t[1]:8.4f} {nbytes / (t[1] * 1e-3) / 1e9:7.0f} | {t[1] / t[0]:11.2f}")

    # ---- rotary of q and k ---------------------------------------------------------------------------------------------------------------
    for label, B, N in (() if a.only_ex else (("prefill 4 x 4096", 4, 4096), ("decode B = 64, one row", 64, 1))):
        q = torch.empty((B, N, H, D), dtype=DT, device=dev).normal_(0, 1.0)
        k = torch.empty((B, N, HK, D), dtype=DT, device=dev).normal_(0, 0.5)
        qo, ko = torch.empty_like(q), torch.empty_like(k)
        lens = torch.randint(0, RO - N, (B,), generator=torch.Generator().manual_seed(B)).to(torch.int32).to(dev)
        pos = (lens.long()[:, None] + torch.arange(N, device=dev)[None, :]).reshape(-1)
        nbytes = 2.0 * (q.numel() + k.numel()) * 2 + 2.0 * B * N * (D // 2) * 2
        for interleaved in (False, True):
            for inplace in (True, False):
                p, keep = ops._rotary_params("bench", (q, k), (q, k) if inplace else (qo, ko), cos, sin, interleaved, False, lens, None)

                def torch_call():
                    rq = torch_rotary(q.view(B * N, H, D), cos, sin, pos, interleaved)
                    rk = torch_rotary(k.view(B * N, HK, D), cos, sin, pos, interleaved)
                    if inplace:
                        q.view(B * N, H, D).copy_(rq)
                        k.view(B * N, HK, D).copy_(rk)

                t = race(lambda: _lib.check(L.tfa_rotary(C.byref(p), stream)), torch_call)
                row(f"rotary q + k, {label}, {'GPT-J' if interleaved else 'GPT-NeoX'}, {'in place' if inplace else 'out of place'}", nbytes, t)
        del q, k, qo, ko

    emit(f"# tfa_kvcache_append_varlen_ex, H{H} Hk{HK} D{D} rotary_dim {D} bf16 rows, page {PAGE}; HIP events, best of {a.rounds} rounds x {a.iters} calls, "
         "the two arms alternated in one process", ex_lines)
    emit("# fp8: the append into an e4m3 pool against the 16-bit append of the same rows; q=: the append with q rotated in its launch against "
         "tfa_kvcache_append_varlen with tables + tfa_rotary on q in place; GB/s over the bytes the arm must move", ex_lines)
    emit(f"# {'shape':<66} | {'ex ms':>8} {'GB/s':>7} | {'other ms':>8} {'GB/s':>7} | {'other / ex':>10}", ex_lines)

    def ex_row(label, nbytes, t):
        emit(f"  {label:<66} | {t[0]:8.4f} {nbytes[0] / (t[0] * 1e-3) / 1e9:7.0f} | {t[1]:8.4f} {nbytes[1] / (t[1] * 1e-3) / 1e9:7.0f} | {t[1] / t[0]:10.2f}", ex_lines)

    # ---- the packed append ---------------------------------------------------------------------------------------------------------------
    for label, new in (("prefill mix 56 short + 4 long", mix_lengths("prefill")), ("decode B = 64, one row", [1] * 64)):
        B, total = len(new), sum(new)
        gen = torch.Generator().manual_seed(total)
        cached = torch.randint(0, 4096, (B,), generator=gen)
        mb = max((int(cached[b]) + new[b] + PAGE - 1) // PAGE for b in range(B))
        nb = B * mb
        bt = torch.randperm(nb, generator=gen).view(B, mb).to(torch.int32)
        cu = [0]
        for n in new:
            cu.append(cu[-1] + n)
        k = torch.empty((total, HK, D), dtype=DT, device=dev).normal_(0, 0.5)
        v = torch.empty((total, HK, D), dtype=DT, device=dev).normal_(0, 0.5)
        kp = torch.zeros((nb, PAGE, HK, D), dtype=DT, device=dev)
        vp = torch.zeros((nb, PAGE, HK, D), dtype=DT, device=dev)
        cud, lens, btd = torch.tensor(cu, dtype=torch.int32, device=dev), cached.to(torch.int32).to(dev), bt.to(dev)
        # the torch composition's slot indices: built once on the host (a serving loop builds them every step; that cost is not charged here)
        pages, rows, pos = [], [], []
        for b in range(B):
            for t in range(new[b]):
                pp = int(cached[b]) + t
                pages.append(int(bt[b, pp // PAGE]))
                rows.append(pp % PAGE)
                pos.append(pp)
        idx = (torch.tensor(pages, device=dev), torch.tensor(rows, device=dev))
        posd = torch.tensor(pos, device=dev)
        # ---- tfa_kvcache_append_varlen_ex: the e4m3 pool, and q rotated in the launch
        kp8 = torch.zeros((nb, PAGE, HK, D), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
        vp8 = torch.zeros((nb, PAGE, HK, D), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
        kd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.006, 0.012)
        vd = torch.empty((B, HK), dtype=torch.float32, device=dev).uniform_(0.006, 0.012)
        p8 = _lib.TfaKvcacheFp8()
        p8.format, p8.k_descale, p8.v_descale = _lib.TFA_KV_E4M3, kd.data_ptr(), vd.data_ptr()
        p8.k_descale_stride[0], p8.k_descale_stride[1], p8.v_descale_stride[0], p8.v_descale_stride[1] = HK, 1, HK, 1
        rows16 = 2.0 * (k.numel() + v.numel())                                   # bytes of the 16-bit rows, read once
        tab = 2.0 * total * (D // 2) * 2
        for fused in (False, True):
            pe = ops._append_varlen_params(k, v, kp8, vp8, cud, lens, btd, cos if fused else None, sin if fused else None, False)
            po = ops._append_varlen_params(k, v, kp, vp, cud, lens, btd, cos if fused else None, sin if fused else None, False)
            t = race(lambda: _lib.check(L.tfa_kvcache_append_varlen_ex(C.byref(pe), C.byref(p8), None, stream)),
                     lambda: _lib.check(L.tfa_kvcache_append_varlen(C.byref(po), stream)))
            ex_row(f"fp8 append vs 16-bit append, {label} ({total} rows){', fused RoPE' if fused else ''}",
                   (1.5 * rows16 + (tab if fused else 0.0), 2.0 * rows16 + (tab if fused else 0.0)), t)
        q = torch.empty((total, H, D), dtype=DT, device=dev).normal_(0, 1.0)
        pq = ops._append_varlen_params(k, v, kp, vp, cud, lens, btd, cos, sin, False)
        rq = _lib.TfaAppendQ()
        rq.q, rq.H = q.data_ptr(), H
        rq.q_stride[0], rq.q_stride[1] = q.stride(1), q.stride(0)
        pr, keep = ops._rotary_params("bench", (q,), (q,), cos, sin, False, False, lens, cud)

        def two_launches():
            _lib.check(L.tfa_kvcache_append_varlen(C.byref(pq), stream))
            _lib.check(L.tfa_rotary(C.byref(pr), stream))

        t = race(lambda: _lib.check(L.tfa_kvcache_append_varlen_ex(C.byref(pq), None, C.byref(rq), stream)), two_launches)
        nb_q = 2.0 * rows16 + 2.0 * q.numel() * 2 + tab
        ex_row(f"append with q= vs append + tfa_rotary(q), {label} ({total} rows)", (nb_q, nb_q + tab), t)
        del q, kp8, vp8
        for fused in (() if a.only_ex else (False, True)):
            p = ops._append_varlen_params(k, v, kp, vp, cud, lens, btd, cos if fused else None, sin if fused else None, False)

            def torch_call():
                kp.index_put_(idx, torch_rotary(k, cos, sin, posd, False) if fused else k)
                vp.index_put_(idx, v)

            t = race(lambda: _lib.check(L.tfa_kvcache_append_varlen(C.byref(p), stream)), torch_call)
            nbytes = 2.0 * (k.numel() + v.numel()) * 2 + (2.0 * total * (D // 2) * 2 if fused else 0.0)
            row(f"append, {label} ({total} rows){', fused RoPE' if fused else ''}", nbytes, t)
        del k, v, kp, vp
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.ex_out:
        with open(a.ex_out, "w") as f:
            f.write("\n".join(ex_lines) + "\n")


if __name__ == "__main__":
    main()
