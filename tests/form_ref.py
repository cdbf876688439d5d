"""One fp64 definition of every attention form's forward, backward and per-element backward bound, and the list of cases that
tests/test_forms_bwd_bounds_gpu.py runs on the GPU and tests/test_form_bounds_cpu.py proves on the CPU (tests only).

The score of query row i and key j, in the order the README states:
    x = sc * q.k   ->   softcap * tanh(x / softcap)   ->   - slope[b,h] * |i + (Nk - Nq) - j|   ->   + bias[b,h,i,j]   ->   the window mask
(key j visible to row i iff i + shift - left <= j <= i + shift + right, shift = Nk - Nq, -1 = unbounded).  A row without a finite score has P = 0.
The bound is oracle.attn_bwd_bounds generalised (see bwd_bounds); check_grads applies the project's (B1) and (B2) of tests/test_bwd_gpu.py with it.
"""
import math
import random

import torch

from helpers import ulp16

NEG = -math.inf
BF16, FP16 = torch.bfloat16, torch.float16


def eps16(dtype):
    """include/tfa.h's eps16: 2^-8 (bf16) / 2^-11 (fp16)."""
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def rnd(shape, dtype, seed, std=0.5):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32).normal_(0.0, std, generator=g).to(dtype)


def std_slopes(H, mult=1.0):
    return torch.tensor([mult * 2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)


def eff_window(causal, window):
    return (window[0], 0) if causal else tuple(window)


def window_mask(Nq, Nk, left, right):
    i = torch.arange(Nq).view(-1, 1)
    j = torch.arange(Nk).view(1, -1)
    shift = Nk - Nq
    m = torch.ones(Nq, Nk, dtype=torch.bool)
    if left >= 0:
        m &= j >= i + shift - left
    if right >= 0:
        m &= j <= i + shift + right
    return m


def _f64(t):
    return t.detach().double().cpu()


def _expand_kv(t, H):
    G = H // t.shape[1]
    return t.repeat_interleave(G, dim=1) if G > 1 else t


def scores64(q, k, sc, *, softcap=0.0, slopes=None, bias=None, window=(-1, -1), mut=None):
    """q (B,H,Nq,D), k (B,H,Nk,D) in fp64 (K/V heads already repeated) -> (S, tanh): S (B,H,Nq,Nk) with -inf where masked, tanh = tanh(x / softcap) of the
    scaled scores (None without a cap; 1 - tanh^2 is the cap's derivative).  slopes: (H,) or (B,H); bias: broadcastable to (B,H,Nq,Nk), -inf entries mask.
    mut: what a wrong kernel would do, for the CPU self-test only — {"straight_through"}: the capped values with the identity's gradient; {"alibi_shift0"}: the
    ALiBi distance without Nk - Nq; {"extra_keys": n}: the last n keys given belong to the NEXT sequence and are visible to every row."""
    mut = mut or {}
    B, H, Nq, _ = q.shape
    extra = int(mut.get("extra_keys", 0))
    Nk = k.shape[2] - extra
    shift = Nk - Nq
    x = (q @ k.transpose(-1, -2)) * sc
    th = None
    if softcap:
        th = torch.tanh(x / softcap)
        x = x + (softcap * th - x).detach() if mut.get("straight_through") else softcap * th
    if slopes is not None:
        s = _f64(slopes)
        s = s.view(1, H, 1, 1) if s.dim() == 1 else s.view(B, H, 1, 1)
        i = torch.arange(Nq, dtype=torch.float64).view(-1, 1)
        j = torch.arange(Nk + extra, dtype=torch.float64).view(1, -1)
        x = x - s * (i + (0 if mut.get("alibi_shift0") else shift) - j).abs()
    if bias is not None:
        x = x + _f64(bias)
    m = window_mask(Nq, Nk, *window)
    if extra:
        m = torch.cat([m, torch.ones(Nq, extra, dtype=torch.bool)], dim=1)
    return x.masked_fill(~m, NEG), th


def _probs(s):
    """softmax over keys; a row without a finite score is P = 0 (softmax + nan_to_num would hand autograd a NaN there)."""
    empty = torch.isneginf(s).all(dim=-1, keepdim=True)
    return torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * (~empty), empty


def ref_fwd(q, k, v, sc, **form):
    """q (B,H,Nq,D), k / v (B,Hk,Nk,D), any float dtype -> out64, lse64 (+inf on rows without a finite score), A = P @ |v|."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    k, v = _expand_kv(k, q.shape[1]), _expand_kv(v, q.shape[1])
    s, _ = scores64(q, k, sc, **form)
    p, empty = _probs(s)
    lse = torch.logsumexp(torch.where(empty, torch.zeros_like(s), s), dim=-1).masked_fill(empty.squeeze(-1), math.inf)
    return p @ v, lse, p @ v.abs()


def structure(q, k, sc, **form):
    """Where the definition gives exact zeros: (rows without a finite score (B,H,Nq), keys no row of any of their query heads sees (B,Hk,Nk))."""
    q, k = _f64(q), _f64(k)
    B, H, Nq, _ = q.shape
    Hk, Nk = k.shape[1], k.shape[2]
    s, _ = scores64(q, _expand_kv(k, H), sc, **form)
    fin = torch.isfinite(s)
    return ~fin.any(dim=-1), ~fin.view(B, Hk, H // Hk, Nq, Nk).any(dim=3).any(dim=2)


def ref_grads(q, k, v, dout, sc, **form):
    """fp64 autograd of ref_fwd's out; GQA by repeat_interleave, so dk and dv are summed over a K/V head's query heads by autograd."""
    q64, k64, v64 = (_f64(t).requires_grad_(True) for t in (q, k, v))
    H = q64.shape[1]
    s, _ = scores64(q64, _expand_kv(k64, H), sc, **form)
    p, _ = _probs(s)
    (p @ _expand_kv(v64, H)).backward(_f64(dout))
    return q64.grad, k64.grad, v64.grad


def bwd_bounds(q, k, v, out16, dout, sc, kv_p16=True, **form):
    """oracle.attn_bwd_bounds for every form: the non-cancelling magnitudes (Aq, Ak, Av), shaped like q, k, v, with |grad_kernel - grad_exact| <= eps16 * A.
        dsabs = P o (|dP - delta| + sum_d |dO O16|)      (o (1 - tanh^2(x / c)) under a cap)
        Aq = sc * dsabs @ |K|,   Ak = sc * dsabs^T @ |Q|,   Av = P^T @ |dO|
    delta = sum_d dO O16 with the 16-bit O the forward stored.  eps16 is the unit roundoff of the 16-bit type: ONE rounding of P (for dV) or of dS (for dQ:
    tfa_bwd_kernel.h rounds P (dP - delta) once, P in fp32) moves each term of the sums by a relative eps16 at most, and the 16-bit O moves every dS by
    P * eps16 * sum |dO O|.  Under a cap the kernels round P * (1 - tanh^2) where they rounded P (tfa_bwd_kv_kernel.h: pf = (T)(pr * (q * (2 - q)));
    tfa_bwd_kernel.h: (T)(y * (q * (2 - q)))), so every term carries the factor and the count of roundings is unchanged: no term of its own.
    kv_p16 (the one term oracle.attn_bwd_bounds does not have; False gives exactly that function): the dK/dV launch rounds TWICE on the way to dK —
    tfa_bwd_kv_kernel.h, role 0: pk = (T)fast_exp2(...) (pf under a cap) is handed to role 1 through LDS as 16 bit, role 1: pk = (T)((float)pp * (x - stv)) —
    so each dS term of dK carries 2 eps16 relative, not one: Ak gets sc * (P o |dP - delta| (o (1 - tanh^2)))^T @ |Q| once more.  A key that few rows see (the
    last keys under a causal mask) sums too few terms for the two roundings to average out; Aq and Av are untouched."""
    qf, kf, vf, of, dof = (_f64(t) for t in (q, k, v, out16, dout))
    B, H, Nq, D = qf.shape
    Hk, Nk = kf.shape[1], kf.shape[2]
    G = H // Hk
    ke, ve = _expand_kv(kf, H), _expand_kv(vf, H)
    s, th = scores64(qf, ke, sc, **form)
    p, _ = _probs(s)
    dp = dof @ ve.transpose(2, 3)
    delta = (dof * of).sum(-1, keepdim=True)
    ds_abs = p * ((dp - delta).abs() + (dof * of).abs().sum(-1, keepdim=True))
    if th is not None:
        ds_abs = ds_abs * (1.0 - th * th)
    aq = sc * (ds_abs @ ke.abs())
    ds_k = ds_abs
    if kv_p16:                                              # the second 16-bit rounding of the dK/dV launch: P handed over in 16 bit, then dS rounded
        ds_k = ds_abs + p * (dp - delta).abs() * (1.0 if th is None else 1.0 - th * th)
    ak = sc * (ds_k.transpose(2, 3) @ qf.abs())
    av = p.transpose(2, 3) @ dof.abs()
    if G > 1:
        ak = ak.view(B, Hk, G, Nk, D).sum(2)
        av = av.view(B, Hk, G, Nk, D).sum(2)
    return aq, ak, av


def ratios(grads, ref, bounds, dtype, half_ulp=False):
    """max(|d| / bound) of each gradient: bound = eps16 * A + 1e-6 (B1), plus half an ulp of the 16-bit result (B2) with half_ulp.  The result is the rounded
    fp32 gradient, which (B1) places within b1 of ref: its ulp is taken at |ref| + b1, the largest magnitude it can have — ulp16(ref) is half of that where
    ref lies just under a power of two and the fp32 gradient just above it, and a correctly rounded result then misses a bound built on ulp16(ref)."""
    res = []
    for g, r, A in zip(grads, ref, bounds):
        bound = eps16(dtype) * A + 1e-6
        if half_ulp:
            bound = bound + 0.5 * ulp16((r.abs() + bound).float(), dtype).double() * (1 + 1e-3)
        d = (_f64(g) - r).abs()
        res.append((d / bound).max().item() if d.numel() else 0.0)
    return res


def check_grads(g32, g16, ref, bounds, dtype, label=""):
    """(B1) |g32 - ref| <= b1 = eps16 * A + 1e-6 and (B2) |g16 - ref| <= b1 + half an ulp16 of the result * (1 + 1e-3) (see ratios), element by element, and every
    gradient finite.  g32 or g16 may be None (autograd returns 16-bit gradients only).  Prints max(|d| / bound) per gradient before asserting; returns them."""
    names = ("dq", "dk", "dv")
    out = {}
    for kind, gs, half in (("fp32", g32, False), ("16-bit", g16, True)):
        if gs is None:
            continue
        for n, g in zip(names, gs):
            assert bool(torch.isfinite(g).all()), f"{label} {n} ({kind}): not finite"
        rs = ratios(gs, ref, bounds, dtype, half_ulp=half)
        out[kind] = rs
        print(f"{label} {'bf16' if dtype == torch.bfloat16 else 'fp16'} {kind:6s} max(|d| / bound): " + "  ".join(f"{n} {r:.3f}" for n, r in zip(names, rs)))
    for kind, rs in out.items():
        for n, r in zip(names, rs):
            assert r <= 1.0, f"({'B1' if kind == 'fp32' else 'B2'}) {label} {n}: {kind} gradient is at {r:.3f} of its per-element bound"
    return out


def round16(x, dtype):
    return x.float().to(dtype).double()


def emulate16(q, k, v, dout, sc, dtype, **form):
    """The kernels' algorithm on the CPU, fp64 everywhere except its 16-bit rounding points: P for O and dV, the stored O, and dS — once for dQ
    (round16(P (dP - delta) (1 - tanh^2))), twice for dK (round16(round16(P (1 - tanh^2)) (dP - delta)): the dK/dV launch hands the 16-bit P over).  Returns ((dq, dk, dv), O16).  For the CPU self-test only."""
    qf, kf, vf, dof = (_f64(t) for t in (q, k, v, dout))
    B, H, Nq, D = qf.shape
    Hk, Nk = kf.shape[1], kf.shape[2]
    G = H // Hk
    ke, ve = _expand_kv(kf, H), _expand_kv(vf, H)
    s, th = scores64(qf, ke, sc, **form)
    p, _ = _probs(s)
    p16 = round16(p, dtype)
    o16 = round16(p16 @ ve, dtype)
    dv = p16.transpose(2, 3) @ dof
    delta = (dof * o16).sum(-1, keepdim=True)
    dpd = dof @ ve.transpose(2, 3) - delta
    dfac = 1.0 if th is None else 1.0 - th * th
    ds_q = round16(p * dpd * dfac, dtype)                        # the dQ launch: P stays fp32 until dS is rounded (tfa_bwd_kernel.h)
    ds_k = round16(round16(p * dfac, dtype) * dpd, dtype)        # the dK/dV launch: role 0 hands role 1 the 16-bit P (tfa_bwd_kv_kernel.h)
    dq = sc * (ds_q @ ke)
    dk = sc * (ds_k.transpose(2, 3) @ qf)
    if G > 1:
        dk = dk.view(B, Hk, G, Nk, D).sum(2)
        dv = dv.view(B, Hk, G, Nk, D).sum(2)
    return (dq, dk, dv), o16


# ---- packed variable-length batches -------------------------------------------------------------------------------------------------------
def cu_of(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def seq_view(t, cu, b, extra=0):
    """Sequence b of a packed (total, H, D) tensor as a (1, H, n, D) view (extra: that many rows behind it as well)."""
    return t[int(cu[b]):int(cu[b + 1]) + extra].transpose(0, 1).unsqueeze(0)


def seq_form(form, b):
    """The form of sequence b: row b of (B, H) slopes."""
    f = dict(form)
    if f.get("slopes") is not None and f["slopes"].dim() == 2:
        f["slopes"] = f["slopes"][b]
    return f


# ---- mutants: what a subtly wrong backward would compute (fp64), for the CPU self-test -----------------------------------------------------
MUTANTS = ("wl+1", "wr+1", "alibi_shift0", "slopes_b0", "no_dtanh", "cap*1.02", "bias_row", "bias_kvhead", "next_key")


def mutant_form(form, name, G=1):
    """The form a wrong kernel would have computed.  ("next_key" needs one more key row: see mutant_grads.)"""
    f = dict(form)
    w = f.get("window", (-1, -1))
    if name == "wl+1":
        assert w[0] >= 0, "the window has no left edge"
        f["window"] = (w[0] + 1, w[1])
    elif name == "wr+1":
        assert w[1] >= 0, "the window has no right edge"
        f["window"] = (w[0], w[1] + 1)
    elif name == "alibi_shift0":
        assert f.get("slopes") is not None
        f["mut"] = {"alibi_shift0": True}
    elif name == "slopes_b0":
        s = f["slopes"]
        assert s.dim() == 2 and s.shape[0] > 1 and not torch.equal(s[0], s[1])
        f["slopes"] = s[0:1].expand_as(s).contiguous()
    elif name == "no_dtanh":
        assert f.get("softcap")
        f["mut"] = {"straight_through": True}
    elif name == "cap*1.02":
        assert f.get("softcap")
        f["softcap"] = f["softcap"] * 1.02
    elif name == "bias_row":
        f["bias"] = torch.roll(f["bias"], 1, dims=2)
    elif name == "bias_kvhead":
        b = f["bias"]
        assert G > 1 and b.shape[1] > 1, "needs GQA and a bias per query head"
        f["bias"] = b[:, torch.arange(b.shape[1]) // G]
    elif name == "next_key":
        f["mut"] = {"extra_keys": 1}
    else:
        raise KeyError(name)
    return f


def mutant_grads(name, q, k, v, dout, sc, form, k_next=None, v_next=None):
    """fp64 gradients of mutant `name`, shaped like q, k, v.  next_key: k_next / v_next hold one more row (the next sequence's first key)."""
    G = q.shape[1] // k.shape[1]
    f = mutant_form(form, name, G)
    if name == "next_key":
        dq, dk, dv = ref_grads(q, k_next, v_next, dout, sc, **f)
        return dq, dk[:, :, :k.shape[2]], dv[:, :, :k.shape[2]]
    return ref_grads(q, k, v, dout, sc, **f)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# The dQ launch holds 256 query rows per workgroup and streams 64-key tiles, the dK/dV launch holds 192 keys and streams 64-row tiles:
SHAPES = [(192, 192),      # whole blocks only
          (70, 203),       # one ragged block each way, Nq < Nk
          (257, 130),      # one row into the second query block, Nq > Nk
          (320, 385)]      # second blocks on both sides, one key into the third key block
VARLEN_LQ, VARLEN_LK = [300, 1, 257, 0, 64], [300, 90, 200, 7, 64]       # ... plus trailing rows outside every sequence
VARLEN_TAIL = (9, 5)


def _case(id, **kw):
    c = dict(id=id, kind="fixed", dtype=BF16, B=1, H=4, Hk=4, D=64, causal=False, window=(-1, -1), slopes=None, cap=0.0, std=0.5, bias=None, seed=100,
             mutants=[], na=[])
    c.update(kw)
    return c


def _window_mutants(causal, window, Nq, Nk):
    """The edge mutants a window has.  Not applicable (structural): an edge that is unbounded, or lies beyond every row's last / first key (left >= Nk - 1,
    right >= Nq - 1: the wrapper itself calls that unbounded) — there is no key to move it by."""
    l, r = eff_window(causal, window)
    mu, na = [], []
    if 0 <= l < Nk - 1:
        mu.append("wl+1")
    else:
        na.append(("wl+1", "left edge unbounded or beyond the first key"))
    if 0 <= r < Nq - 1:
        mu.append("wr+1")
    else:
        na.append(("wr+1", "right edge unbounded or beyond the last key"))
    return mu, na


def _shift0_applies(causal, window, Nq, Nk):
    """alibi_shift0 is not applicable (structural) at Nq == Nk (shift = 0), and under a right edge of 0 with Nq > Nk: every visible key has i + shift - j >= 0
    and -shift > 0, so dropping the shift moves a row's distances by one constant, which the softmax cancels."""
    if Nq == Nk:
        return False, "Nq == Nk: shift = 0"
    if eff_window(causal, window)[1] == 0 and Nq > Nk:
        return False, "right edge 0 with Nq > Nk: the distances move by a row constant"
    return True, None


def _cases():
    cs = []
    dts, dims, hks = [BF16, FP16], [40, 64, 96, 128], [4, 2, 1]                      # H / Hk in {1, 2, 4}
    # window: nine masks x four shapes; dtype, D and H / Hk rotate so that each value meets each mask and each shape
    wins = [(False, w) for w in [(0, 0), (63, 0), (64, 0), (65, 0), (37, 20), (128, 128), (-1, 64), (64, -1)]] + [(True, (200, 77))]
    n = 0
    for wi, (causal, w) in enumerate(wins):
        for si, (Nq, Nk) in enumerate(SHAPES):
            mu, na = _window_mutants(causal, w, Nq, Nk)
            cs.append(_case(f"win{'c' if causal else ''}{w[0]}_{w[1]}-{Nq}x{Nk}", dtype=dts[(wi + si) % 2], D=dims[(wi + si) % 4], Hk=hks[(wi + 2 * si) % 3],
                            Nq=Nq, Nk=Nk, causal=causal, window=w, seed=100 + n, mutants=mu, na=na[:1]))
            n += 1
    # ALiBi: (H,) / (B,H) / steep / a zero and a negative slope x full / causal / windowed, Nq != Nk (alibi_shift0 is not applicable at Nq == Nk: shift = 0)
    al = [("H", 1, False, (-1, -1), 1), ("BH", 2, True, (-1, -1), 1), ("steep", 1, False, (-1, -1), 2), ("zeroneg", 1, False, (37, 20), 3),
          ("BH", 2, False, (64, 0), 2), ("H", 1, True, (-1, -1), 3), ("steep", 1, True, (-1, -1), 1), ("BH", 2, False, (-1, -1), 3),
          ("BH", 2, True, (-1, -1), 0), ("zeroneg", 2, False, (128, 128), 0), ("H", 2, False, (-1, 64), 2), ("steep", 2, False, (64, -1), 3)]
    for ai, (sl, B, causal, w, si) in enumerate(al):
        Nq, Nk = SHAPES[si]
        ok, why = _shift0_applies(causal, w, Nq, Nk)
        mu = (["alibi_shift0"] if ok else []) + (["slopes_b0"] if sl == "BH" else [])
        na = [] if ok else [("alibi_shift0", why)]
        if eff_window(causal, w) != (-1, -1):
            mu += _window_mutants(causal, w, Nq, Nk)[0]
        cs.append(_case(f"alibi-{sl}{'-c' if causal else ''}{w[0]}_{w[1]}-{Nq}x{Nk}", dtype=dts[ai % 2], D=dims[(ai + 1) % 4], B=B, Hk=hks[ai % 3], Nq=Nq, Nk=Nk,
                        causal=causal, window=w, slopes=sl, seed=200 + ai, mutants=mu, na=na))
    # softcap: mid (5, std 2), saturated (5, std 8), near linear (50, std 0.5) x with / without slopes, with a window
    # (cap * 1.02 moves a mid-regime gradient by a few 1e-3 relative: fp16's bound sees it at >= 10x everywhere, bf16's only where noted.  cap 50 at std 0.5 has
    #  |x / c| < 0.03: 1 - tanh^2 differs from 1 by less than 1e-3, below eps16 of either type — BOTH cap mutants are invisible there by construction (the regime
    #  is in the list to guard the cancellation in 1 - tanh^2 for small arguments), so those two cases carry a window and name its edges)
    near = "near linear: 1 - tanh^2 is within 1e-3 of 1, below eps16"
    sc_ = [(5.0, 2.0, None, False, (-1, -1), 0, FP16), (5.0, 2.0, "BH", True, (-1, -1), 1, FP16), (5.0, 8.0, None, True, (-1, -1), 3, BF16),
           (5.0, 8.0, "H", False, (-1, -1), 2, FP16), (50.0, 0.5, None, False, (37, 20), 1, BF16), (50.0, 0.5, "H", False, (64, 0), 3, FP16),
           (5.0, 2.0, None, False, (37, 20), 2, FP16), (5.0, 2.0, "BH", False, (128, 128), 3, FP16), (5.0, 8.0, None, False, (64, 0), 1, BF16),
           (5.0, 2.0, "zeroneg", True, (200, 77), 0, BF16)]
    for ci, (cap, std, sl, causal, w, si, dt) in enumerate(sc_):
        Nq, Nk = SHAPES[si]
        mu = ["no_dtanh", "cap*1.02"] if cap < 50 else []
        na = [] if cap < 50 else [("no_dtanh", near), ("cap*1.02", near)]
        if sl is not None and _shift0_applies(causal, w, Nq, Nk)[0]:
            mu.append("alibi_shift0")
        if sl == "BH":
            mu.append("slopes_b0")
        if eff_window(causal, w) != (-1, -1):
            mu += _window_mutants(causal, w, Nq, Nk)[0]
        cs.append(_case(f"cap{cap:g}-std{std:g}{'-' + sl if sl else ''}-{'c' if causal else ''}{w[0]}_{w[1]}-{Nq}x{Nk}", dtype=dt, D=dims[(ci + 2) % 4],
                        B=2 if sl == "BH" else 1, Hk=hks[(ci + 1) % 3], Nq=Nq, Nk=Nk, causal=causal, window=w, slopes=sl, cap=cap, std=std, seed=300 + ci,
                        mutants=mu, na=na))
    # bias: the four broadcast shapes x q's dtype / fp32, -inf masks, causal, a window, GQA, an expanded bias, a row stride that forces the wrapper's copy
    bi = [((True, True), False, True, "contig", False, (-1, -1), 0), ((False, True), True, True, "padded", False, (-1, -1), 1),
          ((True, False), False, False, "contig", True, (-1, -1), 2), ((False, False), True, True, "contig", False, (37, 20), 3),
          ((True, True), True, False, "odd", False, (-1, -1), 1), ((False, True), False, True, "expanded", True, (-1, -1), 3),
          ((True, False), True, True, "padded", False, (64, 0), 0), ((False, False), False, False, "expanded", False, (-1, -1), 2),
          ((True, True), False, True, "odd", True, (200, 77), 3), ((True, True), True, True, "padded", False, (128, 128), 2)]
    for ii, (bshape, f32, masked, layout, causal, w, si) in enumerate(bi):
        Nq, Nk = SHAPES[si]
        Hk = [2, 1, 4][ii % 3]
        mu = ["bias_row"] + (["bias_kvhead"] if (bshape[1] and Hk < 4) else [])
        if eff_window(causal, w) != (-1, -1):
            mu += _window_mutants(causal, w, Nq, Nk)[0]
        cs.append(_case(f"bias-{'B' if bshape[0] else '1'}{'H' if bshape[1] else '1'}-{'f32' if f32 else 'q'}{'-inf' if masked else ''}-{layout}{'-c' if causal else ''}"
                        f"{w[0]}_{w[1]}-{Nq}x{Nk}", dtype=dts[ii % 2], D=dims[(ii + 3) % 4], B=2, Hk=Hk, Nq=Nq, Nk=Nk, causal=causal, window=w,
                        bias=dict(shape=bshape, f32=f32, masked=masked, layout=layout), seed=400 + ii, mutants=mu))
    # varlen: each of window, slopes and cap, and all three
    for vi, (w, causal, sl, cap, std) in enumerate([((64, 33), False, None, 0.0, 0.5), ((-1, -1), True, "BH", 0.0, 0.5), ((-1, -1), False, None, 5.0, 2.0),
                                                    ((100, 0), False, "BH", 5.0, 2.0), ((37, 20), False, "H", 0.0, 0.5), ((-1, -1), True, "H", 5.0, 8.0)]):
        mu = ["next_key"] + (["no_dtanh", "cap*1.02"] if cap else []) + (["alibi_shift0"] if sl else []) + (["slopes_b0"] if sl == "BH" else [])
        if eff_window(causal, w) != (-1, -1):
            mu += _window_mutants(causal, w, 300, 300)[0]
        cs.append(_case(f"varlen-w{'c' if causal else ''}{w[0]}_{w[1]}{'-' + sl if sl else ''}{f'-cap{cap:g}' if cap else ''}", kind="varlen", dtype=dts[vi % 2],
                        D=[128, 64, 96, 40][vi % 4], H=4, Hk=[2, 4, 1][vi % 3], lq=VARLEN_LQ, lk=VARLEN_LK, causal=causal, window=w, slopes=sl, cap=cap, std=std,
                        seed=500 + vi, mutants=mu))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"
# one autograd case per form through flash_attn_func, and per packed form through flash_attn_varlen_func
AUTOGRAD_IDS = ["win37_20-320x385", "alibi-BH-1_-1-320x385", "cap5-std2-BH-c-1_-1-70x203", "bias-BH-q-inf-contig-1_-1-192x192",
                "varlen-w64_33", "varlen-wc-1_-1-BH", "varlen-w-1_-1-cap5", "varlen-w100_0-BH-cap5"]
assert all(i in BY_ID for i in AUTOGRAD_IDS)


def sweep_case(seed):
    """test_seeded_sweep's draw: dtype, D (a multiple of 8 in 8..128), H / Hk, B in {1, 2}, Nq and Nk in 1..450, fixed-length or varlen, a random legal
    combination of window, slopes and cap, or (fixed-length only) a bias."""
    r = random.Random(seed)
    dtype = r.choice([BF16, FP16])
    D = 8 * r.randint(1, 16)
    G = r.choice([1, 2, 4])
    Hk = r.choice([1, 2, 3, 4] if G == 1 else [1, 2] if G == 2 else [1])
    B = r.choice([1, 2])
    varlen = r.random() < 0.35
    use_bias = (not varlen) and r.random() < 0.3
    Nq, Nk = r.randint(1, 450), r.randint(1, 450)
    lens = [(r.choice([0, 1] + 6 * [r.randint(1, 450)]), r.randint(1, 450)) for _ in range(B)]
    if not any(a for a, _ in lens):
        lens[0] = (r.randint(1, 450), lens[0][1])           # (a batch without a query row has no gradient to check)
    causal = r.random() < 0.3
    wkind = r.choice(["none", "left", "both", "right", "tiny"])
    w = {"none": (-1, -1), "left": (r.randint(0, 300), 0), "both": (r.randint(0, 200), r.randint(0, 200)), "right": (-1, r.randint(0, 200)),
         "tiny": (r.randint(0, 3), r.randint(0, 3))}[wkind]
    sl = r.choice([None, "H", "BH", "steep", "zeroneg"])
    cap, std = r.choice([(0.0, 0.5), (0.0, 1.0), (5.0, 2.0), (5.0, 8.0), (50.0, 0.5), (20.0, 1.0)])
    bias = None
    if use_bias:
        sl, cap, std = None, 0.0, 0.5
        bias = dict(shape=(r.random() < 0.5, r.random() < 0.5), f32=r.random() < 0.5, masked=r.random() < 0.5, layout=r.choice(["contig", "padded", "odd", "expanded"]))
    elif sl is None and not cap and eff_window(causal, w) == (-1, -1):
        sl = "H"                                            # (at least one form: the plain kernels have their own tests)
    if sl == "BH" and B == 1:
        sl = "H"
    c = _case(f"sweep{seed}", kind="varlen" if varlen else "fixed", dtype=dtype, B=B, H=G * Hk, Hk=Hk, D=D, causal=causal, window=w, slopes=sl, cap=cap, std=std,
              bias=bias, seed=1000 + seed)
    if varlen:
        c.update(lq=[a for a, _ in lens], lk=[b for _, b in lens])
    else:
        c.update(Nq=Nq, Nk=Nk)
    return c


def candidate_mutants(c):
    """Every mutant the forms of a case could have (a drawn case names none: the CPU self-test asks that at least one of these bites)."""
    l, r = eff_window(c["causal"], c["window"])
    mu = (["wl+1"] if l >= 0 else []) + (["wr+1"] if r >= 0 else []) + (["no_dtanh", "cap*1.02"] if c["cap"] else [])
    if c["slopes"] is not None:
        mu += ["alibi_shift0"] + (["slopes_b0"] if c["slopes"] == "BH" else [])
    if c["bias"] is not None:
        mu += ["bias_row"] + (["bias_kvhead"] if c["bias"]["shape"][1] and c["bias"]["layout"] != "expanded" and c["H"] > c["Hk"] else [])
    return mu + (["next_key"] if c["kind"] == "varlen" else [])


def _slopes(kind, B, H):
    if kind is None:
        return None
    if kind == "H":
        return std_slopes(H)
    if kind == "BH":
        return torch.stack([std_slopes(H) * (1.0 + 2.0 * b) for b in range(B)]).flip(1)                # (B, H), another row per batch entry
    if kind == "steep":
        return std_slopes(H, 8.0)
    if kind == "zeroneg":
        return torch.tensor([0.5, 0.0, -0.02, 0.0625][:H], dtype=torch.float32) if H > 1 else torch.tensor([-0.02])
    raise KeyError(kind)


def _bias(spec, B, H, Nq, Nk, dtype, seed):
    """The bias as the test hands it to the wrapper (a CPU tensor, logical shape (B or 1, H or 1, Nq, Nk)): normal(0, 1) in q's dtype or fp32; masked: -inf on
    rows 3 and 64 (fully masked rows), key 5 (a key nobody sees), the last 64-key tile, and a seeded quarter of the rest.  Layouts: contig; padded (row stride Nk
    rounded up to 8: passes through the wrapper); odd (row stride Nk + 3: forces the wrapper's copy); expanded (a (1,1) bias expanded with stride 0)."""
    bd = torch.float32 if spec["f32"] else dtype
    layout = spec["layout"]
    b0, b1 = (B if spec["shape"][0] else 1), (H if spec["shape"][1] else 1)
    if layout == "expanded":
        b0, b1 = 1, 1
    rs = {"contig": Nk, "padded": (Nk + 7) // 8 * 8, "odd": Nk + 3, "expanded": Nk}[layout]
    val = rnd((b0, b1, Nq, Nk), torch.float32, seed, std=1.0)
    if spec["masked"]:
        m = torch.rand((b0, b1, Nq, Nk), generator=torch.Generator().manual_seed(seed + 1)) < 0.25
        for row in (3, 64):
            if row < Nq:
                m[:, :, row, :] = True
        if Nk > 5:
            m[:, :, :, 5] = True
        if Nk > 64:
            m[:, :, :, (Nk - 1) // 64 * 64:] = True
        val = val.masked_fill(m, NEG)
    buf = torch.zeros((b0, b1, Nq, rs), dtype=bd)
    t = buf[..., :Nk]
    t.copy_(val.to(bd))
    if layout == "expanded":
        t = t.expand(B, H, Nq, Nk)
    return t


def bias_to_device(bias, spec, dev):
    """The case's bias on the device IN ITS LAYOUT (Tensor.to would make a padded, odd-strided or expanded tensor contiguous)."""
    if bias is None:
        return None
    if spec["layout"] == "expanded":
        return bias[:1, :1].contiguous().to(dev).expand(bias.shape)
    b0, b1, Nq, Nk = bias.shape
    rs = {"contig": Nk, "padded": (Nk + 7) // 8 * 8, "odd": Nk + 3}[spec["layout"]]
    view = torch.zeros((b0, b1, Nq, rs), dtype=bias.dtype, device=dev)[..., :Nk]
    view.copy_(bias)
    return view


def build(case, dtype=None):
    """The tensors of a case, on the CPU: dict(q, k, v, dout, sc, form (fp64 reference's keywords, the effective window), slopes, bias, ...).  fixed: q (B,H,Nq,D),
    k / v (B,Hk,Nk,D); varlen: packed q (tq,H,D), k / v (tk,Hk,D) with VARLEN_TAIL rows outside every sequence, cu_q, cu_k.  dtype: override (the CPU
    self-test runs every case in both)."""
    c = case
    dt = dtype or c["dtype"]
    B, H, Hk, D, seed, std = c["B"], c["H"], c["Hk"], c["D"], c["seed"], c["std"]
    t = dict(case=c, dtype=dt, sc=1.0 / math.sqrt(D), bias=None)
    if c["kind"] == "varlen":
        B = len(c["lq"])
        t["cu_q"], t["cu_k"] = cu_of(c["lq"]), cu_of(c["lk"])
        tq, tk = sum(c["lq"]) + VARLEN_TAIL[0], sum(c["lk"]) + VARLEN_TAIL[1]
        t["q"], t["k"], t["v"] = rnd((tq, H, D), dt, seed, std), rnd((tk, Hk, D), dt, seed + 1, std), rnd((tk, Hk, D), dt, seed + 2)
        t["dout"] = rnd((tq, H, D), dt, seed + 3)
    else:
        Nq, Nk = c["Nq"], c["Nk"]
        t["q"], t["k"], t["v"] = rnd((B, H, Nq, D), dt, seed, std), rnd((B, Hk, Nk, D), dt, seed + 1, std), rnd((B, Hk, Nk, D), dt, seed + 2)
        t["dout"] = rnd((B, H, Nq, D), dt, seed + 3)
        if c["bias"] is not None:
            t["bias"] = _bias(c["bias"], B, H, Nq, Nk, dt, seed + 4)
    t["B"] = B
    t["slopes"] = _slopes(c["slopes"], B, H)
    t["form"] = dict(softcap=c["cap"], slopes=t["slopes"], bias=t["bias"], window=eff_window(c["causal"], c["window"]))
    return t


def sequences(t):
    """A packed case sequence by sequence: (b, q, k, v, dout as (1,H,n,D) views, form of the sequence, k / v with one more row) for every sequence with rows."""
    for b in range(t["B"]):
        if int(t["cu_q"][b + 1]) == int(t["cu_q"][b]):
            continue
        yield (b, seq_view(t["q"], t["cu_q"], b), seq_view(t["k"], t["cu_k"], b), seq_view(t["v"], t["cu_k"], b), seq_view(t["dout"], t["cu_q"], b),
               seq_form(t["form"], b), seq_view(t["k"], t["cu_k"], b, 1), seq_view(t["v"], t["cu_k"], b, 1))
