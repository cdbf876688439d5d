"""All 256 e4m3 codes through the fp8 K/V-cache kernel against torch's decode (needs a GPU).  Two sequences of one key each hold the codes 0..255 along the head
dim of K and of V, the two NaN codes (0x7f, 0xff) replaced by 0x00 — a NaN anywhere in the key would make every score of the row NaN; 128 one-hot query rows make
row i's LSE equal dec(k[i]) and — one key, P = 1 — out equal dec(v).  The NaN codes get keys of their own in a second call: behind a sequence's length they must not reach the
result (checked); what a NaN code gives as the only VALID key of a sequence is printed for information — unspecified, a cache holds none in front of its length.  Prints every code whose decode differs from torch's; exit status 1 if any does.
usage: python tools/probe_kv8_codes.py [--dtype bf16|f16]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tiny_flash_attention_amd as tfa  # noqa: E402

E4M3 = torch.float8_e4m3fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[ap.parse_args().dtype]
    dev = "cuda:0"
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(E4M3).float()
    nan_codes = [c for c in range(256) if want[c].item() != want[c].item()]
    assert nan_codes == [0x7F, 0xFF]
    held = codes.clone()
    held[nan_codes] = 0
    k8 = held.view(2, 1, 1, 128).view(E4M3).to(dev)
    q = torch.eye(128, dtype=dtype).view(1, 128, 1, 128).repeat(2, 1, 1, 1).contiguous().to(dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    out, lse = tfa.flash_attn_with_kvcache(q, k8, k8, cache_seqlens=lens, softmax_scale=1.0, num_splits=1, return_softmax_lse=True)
    torch.cuda.synchronize()
    got_k = lse.cpu().view(256)                          # (B, H = 1, Nq = 128): row i of sequence b pins code 128 b + i of K
    got_v = out.float().cpu()[:, 0, 0, :].reshape(256)   # one key, P = 1: every row's out is dec(v)
    bad = 0
    for c in range(256):
        if c in nan_codes:
            continue
        w, gk, gv = want[c].item(), got_k[c].item(), got_v[c].item()
        if abs(gk - w) > abs(w) * 2.0 ** -20 + 1e-7 or gv != w:      # (the LSE carries the softmax's own fp32 rounding; neighbouring codes are 2^-4 relative apart)
            print(f"code 0x{c:02x}: torch {w!r}, through K (lse) {gk!r}, through V (out) {gv!r}")
            bad += 1
    print(f"{256 - len(nan_codes)} finite codes, {bad} differ from torch's decode")
    # the NaN codes: sequence 0 has 0x7f as its only key, sequence 1 the code of 1.0 (0x38) as its only key and 0xff behind its length
    for code in nan_codes:
        kn = torch.zeros(2, 64, 1, 128, dtype=torch.uint8)
        kn[0, 0] = code
        kn[1, 0] = 0x38
        kn[1, 1:] = code
        kn = kn.view(E4M3).to(dev)
        out, lse = tfa.flash_attn_with_kvcache(q, kn, kn, cache_seqlens=lens, softmax_scale=1.0, num_splits=1, return_softmax_lse=True)
        torch.cuda.synchronize()
        only, behind = lse[0].cpu(), lse[1].cpu()
        ok_behind = bool((behind == 1.0).all()) and bool((out[1].float().cpu() == 1.0).all())
        print(f"code 0x{code:02x}: as the only key -> lse {only[0, 0].item()!r} (for information); "
              f"behind the length -> {'not read' if ok_behind else 'REACHED THE RESULT: ' + repr(behind[0, :4].tolist())}")
        bad += 0 if ok_behind else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
