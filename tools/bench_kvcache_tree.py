"""A tree mask over the step's new keys against the plain causal call: tfa_fwd_kvcache_tree (flash_attn_with_kvcache(tree_mask=)) with seeded random-tree words
against the plain causal entry point of the same library on the same cache at the SAME split count — the plain call timed twice per round: its own repeat spread;
never the tree call against itself.  H32 Hk8 D128 bf16 q, 256-key pages reached through a shuffled block table, 16384 keys per sequence (the new keys included),
pack_gqa on (tfa_fwd_kvcache_pack with TFA_PACK_GQA_ON as the baseline), Nq in {8, 32, 64}, B in {1, 8, 64}, a bf16 and an e4m3 cache.
Through the C ABI with prebuilt parameter blocks; times are HIP events around `iters` back-to-back calls (after warm-up calls), best of `--rounds` rounds, the arms
alternated in one process.
Expectation, written down before any measurement: the mask removes no tile; at most two 64-key tiles per chunk take the longer masked tile body and every row loads
two dwords once per query block, so the tree call should sit within the plain arm's repeat spread plus that — a fraction of a percent at 256 tiles per sequence.
usage: python tools/bench_kvcache_tree.py [--batches 1,8,64] [--rows 8,32,64] [--iters 10] [--rounds 3] [--out profiles/kvcache_tree_bench.txt] [--readme README.md]
       python tools/bench_kvcache_tree.py --from profiles/kvcache_tree_bench.txt --readme README.md      (no GPU: the README block of an earlier run)"""
import argparse
import ctypes as C
import math
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HK, D, PAGE, KEYS = 32, 8, 128, 256, 16384
SCALE = 1.0 / math.sqrt(D)
OPEN, CLOSE = "<!-- kvcache-tree-measured -->", "<!-- /kvcache-tree-measured -->"
ROW = re.compile(r"^(bf16|e4m3) B (\d+) Nq (\d+) splits (\d+): plain ([\d.]+) / ([\d.]+) us, tree ([\d.]+) us, ([\d.]+) x")


def tree_words(B, nq, seed):
    """parent[t] uniform in [-1, t), word[t] = word[parent] | 1 << t: one seeded random tree per sequence, as signed 64-bit words."""
    r = random.Random(seed)
    out = []
    for _ in range(B):
        ws = []
        for t in range(nq):
            par = r.randint(-1, t - 1)
            ws.append((ws[par] if par >= 0 else 0) | 1 << t)
        out.append([w - (1 << 64) if w >> 63 else w for w in ws])
    return out


def readme_block(lines):
    rows = [m.groups() for m in map(ROW.match, lines) if m]
    if not rows:
        return f"{OPEN}\nNot measured yet: `tools/bench_kvcache_tree.py` writes `profiles/kvcache_tree_bench.txt`.\n{CLOSE}"
    txt = [OPEN,
           f"Measured on MI355X, H{H} Hk{HK} D{D} bf16 q, {PAGE}-key pages through a shuffled block table, {KEYS} keys per sequence, `pack_gqa` on, C ABI with prebuilt",
           "parameter blocks, HIP events, best of 3 rounds × 10 calls unless the file says otherwise, the arms alternated in one process (`tools/bench_kvcache_tree.py`,",
           "`profiles/kvcache_tree_bench.txt`). Both arms ran at the plain call's suggested split count (in brackets); the tree arm's words are seeded random trees:",
           "",
           "| cache | B | Nq | plain causal, run 1 / run 2 (µs) | `tree_mask` (µs) | × plain |",
           "|---|---|---|---|---|---|"]
    for cache, B, nq, s, p1, p2, tr, x in rows:
        txt.append(f"| {cache} | {B} | {nq} | {p1} / {p2} [{s}] | {tr} | {x} |")
    xs = [float(r[7]) for r in rows]
    spread = max(abs(float(r[5]) / float(r[4]) - 1.0) for r in rows)
    txt += ["",
            f"The tree call took {min(xs):.3f}–{max(xs):.3f} × the plain call's time over these {len(rows)} shapes; the plain call's own two runs differ by up to "
            f"{100 * spread:.1f} %. Only these shapes were measured.",
            CLOSE]
    return "\n".join(txt)


def write_readme(path, lines):
    s = open(path).read()
    i, j = s.index(OPEN), s.index(CLOSE) + len(CLOSE)
    open(path, "w").write(s[:i] + readme_block(lines) + s[j:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--rows", default="8,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None, help="rewrite the kvcache-tree-measured block of this README from the run (or from --from)")
    ap.add_argument("--from", dest="src", default=None, help="an earlier result file: no measurement")
    a = ap.parse_args()
    if a.src:
        write_readme(a.readme, open(a.src).read().splitlines())
        return
    import torch

    from tiny_flash_attention_amd import _lib
    from tools.bench_kvcache_window import cache_block, pool, race

    ON = _lib.TFA_PACK_GQA_ON
    L = _lib.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# a tree mask over the new keys of a K/V cache: H{H} Hk{HK} D{D} bf16 q, page {PAGE}, {KEYS} keys, pack_gqa on; tfa_fwd_kvcache_tree (seeded random trees) vs")
    emit(f"# the plain causal call (twice: its repeat spread) at the same split count; HIP events, best of {a.rounds} rounds x {a.iters} calls, arms alternated")
    for fp8 in (False, True):
        for B in (int(b) for b in a.batches.split(",")):
            mb = KEYS // PAGE
            kc, vc = pool(B * mb, fp8, dev), pool(B * mb, fp8, dev)
            bt = torch.randperm(B * mb, generator=torch.Generator().manual_seed(99)).view(B, mb).to(torch.int32).to(dev)
            lens_d = torch.full((B,), KEYS, dtype=torch.int32, device=dev)
            for nq in (int(n) for n in a.rows.split(",")):
                q = torch.empty((B, nq, H, D), dtype=torch.bfloat16, device=dev).normal_(0, 1.0)
                words = torch.tensor(tree_words(B, nq, 17 * B + nq), dtype=torch.int64).to(dev)
                ps = []
                for _ in range(2):
                    o, l = torch.empty((B, H, nq, D), dtype=torch.bfloat16, device=dev), torch.empty((B, H, nq), dtype=torch.float32, device=dev)
                    p = _lib.TfaKvcacheParams()
                    p.q, p.out, p.lse = q.data_ptr(), o.data_ptr(), l.data_ptr()
                    p.B, p.H, p.Hk, p.Nq, p.D = B, H, HK, nq, D
                    p.q_stride[0], p.q_stride[1], p.q_stride[2] = nq * H * D, D, H * D
                    p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * nq * D, nq * D, D
                    cache_block(p, kc, vc, bt, lens_d, KEYS)
                    ps.append((p, o, l))
                p8 = _lib.TfaKvcacheFp8()
                p8.format = _lib.TFA_KV_E4M3
                q8 = C.byref(p8) if fp8 else None
                tr = _lib.TfaKvcacheTree()
                tr.mask, tr.batch_stride, tr.row_stride = words.data_ptr(), words.stride(0), words.stride(1)
                s0 = L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(ps[0][0]), ON)
                assert s0 == L.tfa_fwd_kvcache_tree_suggest_splits(C.byref(ps[1][0]), None, ON, C.byref(tr))
                need = max(L.tfa_fwd_kvcache_pack_workspace(C.byref(ps[0][0]), q8, ON, s0), L.tfa_fwd_kvcache_tree_workspace(C.byref(ps[1][0]), None, q8, ON, C.byref(tr), s0))
                if need < 0:
                    _lib.check(int(need))
                ws = torch.empty((max(int(need), 4),), dtype=torch.float32, device=dev)
                plain = lambda: _lib.check(L.tfa_fwd_kvcache_pack(C.byref(ps[0][0]), q8, ON, s0, ws.data_ptr(), stream))      # noqa: E731
                tree = lambda: _lib.check(L.tfa_fwd_kvcache_tree(C.byref(ps[1][0]), None, q8, ON, C.byref(tr), s0, None, ws.data_ptr(), stream))      # noqa: E731
                best = race([("plain", plain), ("plain again", plain), ("tree", tree)], a.rounds, a.iters)
                gb = 2.0 * B * HK * KEYS * D * (1 if fp8 else 2) / 1e9
                emit(f"{'e4m3' if fp8 else 'bf16'} B {B} Nq {nq} splits {s0}: plain {best[0] * 1e3:.1f} / {best[1] * 1e3:.1f} us, tree {best[2] * 1e3:.1f} us, "
                     f"{best[2] / best[0]:.3f} x the plain call's time   ({gb / (best[0] * 1e-3):.0f} / {gb / (best[2] * 1e-3):.0f} GB/s of K/V bytes)")
            del kc, vc
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.readme:
        write_readme(a.readme, lines)


if __name__ == "__main__":
    main()
