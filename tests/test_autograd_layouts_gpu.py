"""The three autograd functions (flash_attn_func, flash_attn_varlen_func, apply_rotary_emb) on the tensors a training loop hands them: upstream gradients as the
consumers of ``out`` leave them (expanded with stride 0, sliced out of a torch.cat at an odd stride and a misaligned base, transposed, permuted), inputs that
are views of shared projection leaves, and autograd's own modes (partial requires_grad, repeated backward, checkpointing, no-grad, graph capture, second
derivatives).  tests/autograd_layouts.py holds the catalogues; tests/test_autograd_layouts_cpu.py proves on the CPU that torch hands the strides they claim.

No new tolerance.  Every assertion is (1) bit equality with the same call on contiguous, aligned clones and the dense gradient — the backward is deterministic
and layout-independent (tests/test_bwd_gpu.py: test_bwd_strided_bnhd_matches_bhnd) — or (2) an existing bound: form_ref.check_grads' (B2) against fp64 with
form_ref.bwd_bounds on the stored 16-bit out, and rotary_ref.excess <= 0.  check_grads prints max(|d| / bound) per gradient before it asserts.
"""
import functools
import math

import pytest
import torch

import autograd_layouts as AL
import form_ref as F
import rotary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TFA_ERR_STRIDE, TFA_ERR_ALIGN = -5, -6                       # include/tfa.h
B, H, HK = 2, 4, 2


@pytest.fixture(scope="module")
def tfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import tiny_flash_attention_amd as m
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    return m


def bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- the function configurations ---------------------------------------------------------------------------------------------------------------
def _cfg(id, **kw):
    return F._case(id, B=B, H=H, Hk=HK, **kw)


def _form(case_id):
    """A case of form_ref.AUTOGRAD_IDS — its form, dtype, head dim and shape — at this file's B, H, Hk."""
    assert case_id in F.AUTOGRAD_IDS
    return dict(F.BY_ID[case_id], B=B, H=H, Hk=HK)


FIXED = {c["id"]: c for c in (
    _cfg("plain-bf16-d128-c-70x203", dtype=F.BF16, D=128, causal=True, Nq=70, Nk=203, seed=600),
    _cfg("plain-fp16-d64-257x130", dtype=F.FP16, D=64, causal=False, Nq=257, Nk=130, seed=610),
    _cfg("plain-bf16-d192-c-200x333", dtype=F.BF16, D=192, causal=True, Nq=200, Nk=333, seed=620),      # the 256-wide kernels: three gradient launches
    _form("win37_20-320x385"), _form("cap5-std2-BH-c-1_-1-70x203"), _form("bias-BH-q-inf-contig-1_-1-192x192"))}
PLAIN = "plain-bf16-d128-c-70x203"
WINDOWED = "win37_20-320x385"
VARLEN = {c["id"]: c for c in (
    F._case("varlen-plain-c", kind="varlen", dtype=F.BF16, D=128, H=H, Hk=HK, lq=F.VARLEN_LQ, lk=F.VARLEN_LK, causal=True, seed=630),
    dict(F.BY_ID["varlen-w64_33"], H=H, Hk=HK))}
VARLEN_PLAIN = "varlen-plain-c"
ROTARY = {"neox-4d": (torch.bfloat16, False, False), "gptj-4d": (torch.float16, True, False),
          "neox-packed-offsets": (torch.bfloat16, False, True), "gptj-packed-offsets": (torch.float16, True, True)}
RO, RD, RD_D, RN = 80, 32, 64, 70
R_CU, R_TOTAL, R_OFF = [0, 0, 1, 66, 73], 76, [5, 0, 20, 78]

FOUR = AL.RAISED + ("sum_batch",)                             # on the other configurations: the three that used to raise, and a zero batch stride
FOUR_PACKED = AL.RAISED + ("sum_heads",)                      # (a packed batch has no batch dim: the zero head stride)


@functools.lru_cache(maxsize=None)
def problem(cfg_id):
    """The configuration's CPU tensors (form_ref.build): computed once, shared, never modified."""
    return F.build(FIXED[cfg_id] if cfg_id in FIXED else VARLEN[cfg_id])


def attention(tfa, t):
    """(f(q, k, v) -> out, fresh leaves on the device in the function's layout) of an attention configuration."""
    c = t["case"]
    kw = dict(window_size=c["window"], softcap=c["cap"], alibi_slopes=None if t["slopes"] is None else t["slopes"].to(DEV))
    if c["kind"] == "varlen":
        cu = (t["cu_q"].to(DEV), t["cu_k"].to(DEV), max(c["lq"]), max(c["lk"]))
        return (lambda q, k, v: tfa.flash_attn_varlen_func(q, k, v, *cu, causal=c["causal"], **kw)), lambda: tuple(
            t[n].to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    if t["bias"] is not None:
        kw["attn_bias"] = F.bias_to_device(t["bias"], c["bias"], DEV)
    return (lambda q, k, v: tfa.flash_attn_func(q, k, v, causal=c["causal"], **kw)), lambda: tuple(
        t[n].transpose(1, 2).contiguous().to(DEV).requires_grad_(True) for n in ("q", "k", "v"))


def rotary(tfa, cfg_id):
    """(f(x) -> out, a fresh leaf, (cos, sin, pos, valid, interleaved, dtype) for the fp64 reference) of a rotary configuration."""
    dtype, interleaved, packed = ROTARY[cfg_id]
    cos, sin = R.tables(RO, RD, dtype)
    cd, sd = cos.to(DEV), sin.to(DEV)
    if packed:
        kw = dict(cu_seqlens=torch.tensor(R_CU, dtype=torch.int32, device=DEV), seqlen_offsets=torch.tensor(R_OFF, dtype=torch.int32, device=DEV))
        shape, (pos, valid) = (R_TOTAL, H, RD_D), R.packed_positions(R_TOTAL, R_CU, R_OFF)
    else:
        kw = dict(seqlen_offsets=15)
        shape, pos, valid = (B, RN, H, RD_D), R.positions(B, RN, 15), None
    x = F.rnd(shape, dtype, 640, 1.0)
    return (lambda x: tfa.apply_rotary_emb(x, cd, sd, interleaved=interleaved, **kw)), (lambda: (x.to(DEV).requires_grad_(True),)), \
        (cos, sin, pos, valid, interleaved, dtype)


def through_consumer(f, inputs, consumer, g):
    """out = f(*inputs); consumer(out).backward(g).  Returns (out, the gradient autograd handed ``out``, a copy of its bits taken when it was handed over)."""
    out = f(*inputs)
    seen = {}

    def hook(grad):
        seen["dout"], seen["bits"] = grad, grad.clone(memory_format=torch.contiguous_format)

    out.register_hook(hook)
    consumer.y(out).backward(g)
    return out, seen["dout"], seen["bits"]


def consumer_vs_dense(f, leaves, cid, seed=650):
    """One consumer against the dense control.  Returns (out, the leaves of the strided run, the dense gradient on the CPU, the handed gradient)."""
    inputs = leaves()
    shape = tuple(inputs[0].shape)                           # (out is shaped like q / x)
    consumer = AL.catalogue(shape)[cid]
    g = AL.upstream(consumer, shape, inputs[0].dtype, seed)
    dense = AL.dense_dout(consumer, shape, g)
    out, dout, handed = through_consumer(f, inputs, consumer, g.to(DEV))
    torch.cuda.synchronize()
    assert (tuple(dout.stride()), dout.storage_offset()) == consumer.strides(*shape), f"{cid}: autograd handed another layout than the catalogue claims"
    assert same(dout, handed) and same(dout, dense), f"{cid}: the handed gradient was written (or is not the dense one)"
    control = leaves()
    f(*control).backward(dense.to(DEV))
    torch.cuda.synchronize()
    for n, a, b in zip("qkv", inputs, control):
        assert a.grad is not None and same(a.grad, b.grad), f"{cid}: the gradient of input {n} differs from the run on the dense upstream gradient"
    return out, inputs, dense, dout


# ---- (a) consumers x functions -------------------------------------------------------------------------------------------------------------------
ATTN_A = ([(PLAIN, c.id) for c in AL.CONSUMERS] + [(cfg, c) for cfg in FIXED if cfg != PLAIN for c in FOUR] +
          [(VARLEN_PLAIN, c.id) for c in AL.PACKED_CONSUMERS] + [(cfg, c) for cfg in VARLEN if cfg != VARLEN_PLAIN for c in FOUR_PACKED])


@pytest.mark.parametrize("cfg_id,cid", ATTN_A, ids=[f"{a}-{b}" for a, b in ATTN_A])
def test_attention_consumer_matches_dense_dout(tfa, monkeypatch, cfg_id, cid):
    """q.grad, k.grad, v.grad are the bits of out.backward(dense dout); the handed gradient keeps its bits; a layout the C ABI takes reaches the kernels
    uncopied, any other as one contiguous, aligned copy."""
    from tiny_flash_attention_amd import ops

    t = problem(cfg_id)
    name = "flash_attn_varlen_bwd" if t["case"]["kind"] == "varlen" else "flash_attn_bwd"
    real, got = getattr(ops, name), []

    def spy(*a, **kw):
        got.append(a[5])
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, spy)
    f, leaves = attention(tfa, t)
    _, _, _, dout = consumer_vs_dense(f, leaves, cid)
    assert len(got) == 2
    k_dout = got[0]                                          # what the strided run's backward gave the kernels
    if AL.abi_takes(tuple(dout.stride()), dout.storage_offset(), dout.shape[-1]):
        assert k_dout.data_ptr() == dout.data_ptr() and k_dout.stride() == dout.stride(), f"{cid}: a layout the kernels take was copied"
    else:
        assert k_dout.is_contiguous() and k_dout.data_ptr() % 16 == 0 and k_dout.data_ptr() != dout.data_ptr()


ROT_A = [(cfg, c.id) for cfg, (_, _, packed) in ROTARY.items() for c in (AL.PACKED_CONSUMERS if packed else AL.CONSUMERS)]


@pytest.mark.parametrize("cfg_id,cid", ROT_A, ids=[f"{a}-{b}" for a, b in ROT_A])
def test_rotary_consumer_matches_dense_dout(tfa, cfg_id, cid):
    f, leaves, _ = rotary(tfa, cfg_id)
    consumer_vs_dense(f, leaves, cid)


def check_fixed_b2(label, t, q, k, v, out, dout, grads):
    """(B2) of a (B, N, H, D) call against fp64: everything on the CPU as (B, H, N, D)."""
    tr = lambda x: x.detach().cpu().transpose(1, 2)          # noqa: E731
    q, k, v, o, do = (tr(x) for x in (q, k, v, out, dout))
    F.check_grads(None, tuple(tr(g) for g in grads), F.ref_grads(q, k, v, do, t["sc"], **t["form"]), F.bwd_bounds(q, k, v, o, do, t["sc"], **t["form"]),
                  t["dtype"], label)


@pytest.mark.parametrize("cfg_id", list(FIXED) + list(VARLEN))
def test_attention_strided_dout_vs_fp64(tfa, cfg_id):
    """Once per configuration: the gradients of the run whose upstream gradient came out of the torch.cat (odd row stride, misaligned base) meet (B2) against
    fp64 on the dense gradient."""
    t = problem(cfg_id)
    f, leaves = attention(tfa, t)
    out, (q, k, v), dense, _ = consumer_vs_dense(f, leaves, "cat_flat_front4")
    if t["case"]["kind"] != "varlen":
        check_fixed_b2(cfg_id, t, q, k, v, out, dense, (q.grad, k.grad, v.grad))
        return
    cq, ck = t["cu_q"], t["cu_k"]
    o, gq, gk, gv = out.detach().cpu(), q.grad.cpu(), k.grad.cpu(), v.grad.cpu()
    for b, qs, ks, vs, _, form, _, _ in F.sequences(t):
        gs = (F.seq_view(gq, cq, b), F.seq_view(gk, ck, b), F.seq_view(gv, ck, b))
        if ks.shape[2] == 0:
            assert all(bool((g == 0).all()) for g in gs)
            continue
        do = F.seq_view(dense, cq, b)
        F.check_grads(None, gs, F.ref_grads(qs, ks, vs, do, t["sc"], **form), F.bwd_bounds(qs, ks, vs, F.seq_view(o, cq, b), do, t["sc"], **form), t["dtype"],
                      f"{cfg_id}[seq {b}]")
    for g, n in ((gq, int(cq[-1])), (gk, int(ck[-1])), (gv, int(ck[-1]))):
        assert bool((g[n:] == 0).all()), "rows outside every sequence must have exactly zero gradients"


@pytest.mark.parametrize("cfg_id", list(ROTARY))
def test_rotary_strided_dout_vs_fp64(tfa, cfg_id):
    f, leaves, (cos, sin, pos, valid, interleaved, dtype) = rotary(tfa, cfg_id)
    _, (x,), dense, _ = consumer_vs_dense(f, leaves, "cat_flat_front4")
    ref, mag, _ = R.rotary_ref64(dense.reshape(-1, H, RD_D), cos, sin, pos, interleaved, conjugate=True, valid=valid)
    e = R.excess(x.grad.cpu().reshape(-1, H, RD_D), ref, mag, dtype)
    print(f"{cfg_id}: excess {e:.3e}")
    assert e <= 0.0, f"a gradient element exceeds the bar by {e:.3e}"


# ---- (b) input views x functions -----------------------------------------------------------------------------------------------------------------
def view_setup(tfa, fn, view):
    """(f, dims, dtype, rows of ``out`` that are written) of an input-view test: plain bf16 D = 128 causal, the (37, 20) window in fp16, or plain packed."""
    if fn == "varlen":
        lens = F.VARLEN_LQ
        total = sum(lens) + F.VARLEN_TAIL[0]
        cu = F.cu_of(lens).to(DEV)
        return (lambda q, k, v: tfa.flash_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=True)), (total, total, H, HK, 128), F.BF16, sum(lens)
    nq, nk = (203, 203) if view.fused else (70, 203)
    if fn == "plain":
        return (lambda q, k, v: tfa.flash_attn_func(q, k, v, causal=True)), (B, nq, nk, H, HK, 128), F.BF16, None
    return (lambda q, k, v: tfa.flash_attn_func(q, k, v, window_size=(37, 20))), (B, nq, nk, H, HK, 128), F.FP16, None


def run_view(tfa, fn, view, seed=700):
    f, dims, dtype, rows = view_setup(tfa, fn, view)
    leaves, qkv, clones = AL.build_view(view, dims, dtype, seed, DEV)
    before = [bits(l) for l in leaves]
    out = f(*qkv)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(l), b) for l, b in zip(leaves, before)), "the forward wrote into its inputs' leaf"
    do = F.rnd(tuple(out.shape), dtype, seed + 50).to(DEV)
    out.backward(do)
    out_c = f(*clones)
    out_c.backward(do)
    torch.cuda.synchronize()
    assert same(out[:rows], out_c[:rows]), f"{view.id}: out differs from the run on contiguous clones"
    for l, want in zip(leaves, AL.assemble(view, dims, leaves, tuple(c.grad for c in clones))):
        assert same(l.grad, want), f"{view.id}: a leaf's gradient differs from the one assembled from the contiguous run"
    return leaves, qkv, out, do


VIEWS_B = [(fn, v.id) for fn in ("plain", "window") for v in AL.INPUT_VIEWS] + [("varlen", v.id) for v in AL.PACKED_INPUT_VIEWS]


@pytest.mark.parametrize("fn,vid", VIEWS_B, ids=[f"{a}-{b}" for a, b in VIEWS_B])
def test_input_views_match_contiguous_clones(tfa, fn, vid):
    run_view(tfa, fn, (AL.PACKED_VIEW_BY_ID if fn == "varlen" else AL.VIEW_BY_ID)[vid])


def test_qkv3_views_vs_fp64(tfa):
    leaves, (q, k, v), out, do = run_view(tfa, "plain", AL.VIEW_BY_ID["qkv3"])
    t = dict(sc=1.0 / math.sqrt(128), dtype=F.BF16, form=dict(window=(-1, 0)))
    check_fixed_b2("qkv3 views", t, q, k, v, out, do, leaves[0].grad.unbind(2))


# ---- (c) autograd's own modes, on the plain D = 128 case -------------------------------------------------------------------------------------------
def plain_run(tfa):
    t = problem(PLAIN)
    f, leaves = attention(tfa, t)
    do = t["dout"].transpose(1, 2).contiguous().to(DEV)
    inputs = leaves()
    out = f(*inputs)
    out.backward(do)
    return f, leaves, do, out, inputs


@pytest.mark.parametrize("which", ["q", "kv"])
def test_partial_requires_grad(tfa, which):
    f, leaves, do, _, full = plain_run(tfa)
    q, k, v = (x.detach().requires_grad_((n == "q") == (which == "q")) for n, x in zip("qkv", leaves()))
    f(q, k, v).backward(do)
    torch.cuda.synchronize()
    for x, ref in zip((q, k, v), full):
        assert (x.grad is None) if not x.requires_grad else same(x.grad, ref.grad)


def test_repeated_backward_accumulates(tfa):
    f, leaves, do, _, full = plain_run(tfa)
    inputs = leaves()
    out = f(*inputs)
    out.backward(do, retain_graph=True)
    out.backward(do, retain_graph=True)
    torch.cuda.synchronize()
    for x, ref in zip(inputs, full):
        assert same(x.grad, ref.grad * 2)


def test_checkpoint_gives_the_same_bits(tfa):
    from torch.utils.checkpoint import checkpoint

    f, leaves, do, out, full = plain_run(tfa)
    inputs = leaves()
    out_c = checkpoint(f, *inputs, use_reentrant=False)
    out_c.backward(do)
    torch.cuda.synchronize()
    assert same(out_c, out)
    for x, ref in zip(inputs, full):
        assert same(x.grad, ref.grad)


def test_no_grad_modes_give_the_forward_bits(tfa):
    f, leaves, _, out, _ = plain_run(tfa)
    inputs = leaves()
    with torch.no_grad():
        a = f(*inputs)
    with torch.inference_mode():
        b = f(*inputs)
    torch.cuda.synchronize()
    assert not a.requires_grad and not b.requires_grad and same(a, out) and same(b, out)


def test_graph_capture_of_forward_and_backward(tfa):
    """One captured forward + backward: a qkv3 leaf, the sum_rows consumer (its gradient is copied inside the capture).  Refilled in place and replayed, the
    leaf's gradient has the eager bits."""
    view, dims, consumer = AL.VIEW_BY_ID["qkv3"], (B, 203, 203, H, H, 128), AL.BY_ID["sum_rows"]
    g = AL.upstream(consumer, (B, 203, H, 128), F.BF16, 720).to(DEV)
    f = lambda q, k, v: tfa.flash_attn_func(q, k, v, causal=True)          # noqa: E731

    def step(leaf):
        consumer.y(f(*view.views([leaf], *dims))).backward(g)

    first, second = (F.rnd(view.leaves(*dims)[0], F.BF16, s).to(DEV) for s in (721, 722))
    want = second.clone().requires_grad_(True)
    step(want)
    leaf = first.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up off the default stream, as graph capture of autograd wants it
        step(leaf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    leaf.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(leaf)
    with torch.no_grad():
        leaf.copy_(second)
        leaf.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same(leaf.grad, want.grad)


SECOND = ["flash_attn_func", "flash_attn_varlen_func", "apply_rotary_emb"]


@pytest.mark.parametrize("loss_kind", ["linear", "quadratic"])
@pytest.mark.parametrize("fn", SECOND)
def test_second_derivatives_raise(tfa, fn, loss_kind):
    """The gradients come out of kernel launches with no graph behind them: under create_graph=True, differentiating anything that depends on them must raise,
    not treat them as constants — also under a linear loss, whose upstream gradient requires no grad while dq still depends on q, k, v."""
    if fn == "apply_rotary_emb":
        f, leaves, _ = rotary(tfa, "neox-4d")
    else:
        f, leaves = attention(tfa, problem(PLAIN if fn == "flash_attn_func" else VARLEN_PLAIN))
    inputs = leaves()
    out = f(*inputs)
    w = F.rnd(tuple(out.shape), torch.float32, 730).to(DEV)
    loss = (out.float() * w).sum() if loss_kind == "linear" else (out.float() * w).pow(2).sum()
    (g,) = torch.autograd.grad(loss, inputs[0], create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        (loss + g.float().pow(2).sum()).backward()             # a gradient penalty


# ---- (d) the chain a model runs --------------------------------------------------------------------------------------------------------------------
def test_projection_rotary_attention_chain(tfa):
    """qkv3 leaf -> apply_rotary_emb on the q and k views -> flash_attn_func(causal) -> the cat_flat_front4 consumer.  Each stage is held to its bound for the
    16-bit tensors it actually saw; the whole chain is the bits of the chain on contiguous clones."""
    N, D, dtype = 203, 128, F.BF16
    view, dims, consumer = AL.VIEW_BY_ID["qkv3"], (B, N, N, H, H, D), AL.BY_ID["cat_flat_front4"]
    cos, sin = R.tables(256, 64, dtype)
    cd, sd = cos.to(DEV), sin.to(DEV)
    g = AL.upstream(consumer, (B, N, H, D), dtype, 740).to(DEV)

    def chain(q, k, v, seen=None):
        qr, kr = tfa.apply_rotary_emb(q, cd, sd), tfa.apply_rotary_emb(k, cd, sd)
        out = tfa.flash_attn_func(qr, kr, v, causal=True)
        if seen is not None:
            seen.update(qr=qr.detach(), kr=kr.detach(), v=v.detach(), out=out.detach())
            for n, x in (("dout", out), ("dqr", qr), ("dkr", kr), ("dv", v), ("dq", q), ("dk", k)):
                x.register_hook(lambda grad, n=n: seen.__setitem__(n, grad.clone(memory_format=torch.contiguous_format)))
        consumer.y(out).backward(g)

    leaves, qkv, clones = AL.build_view(view, dims, dtype, 741, DEV)
    seen = {}
    chain(*qkv, seen=seen)
    chain(*clones)
    torch.cuda.synchronize()
    (want,) = AL.assemble(view, dims, leaves, tuple(c.grad for c in clones))
    assert same(leaves[0].grad, want), "the chain on views of one leaf differs from the chain on contiguous clones"
    assert same(seen["dout"], AL.dense_dout(consumer, (B, N, H, D), g.cpu()))
    t = dict(sc=1.0 / math.sqrt(D), dtype=dtype, form=dict(window=(-1, 0)))
    check_fixed_b2("chain: attention stage", t, seen["qr"], seen["kr"], seen["v"], seen["out"], seen["dout"], (seen["dqr"], seen["dkr"], seen["dv"]))
    pos = R.positions(B, N, 0)
    for n in ("q", "k"):
        ref, mag, _ = R.rotary_ref64(seen[f"d{n}r"].cpu().reshape(-1, H, D), cos, sin, pos, False, conjugate=True)
        e = R.excess(seen[f"d{n}"].cpu().reshape(-1, H, D), ref, mag, dtype)
        print(f"chain: rotary stage d{n} excess {e:.3e}")
        assert e <= 0.0, f"rotary stage d{n}: an element exceeds the bar by {e:.3e}"


# ---- (e) the explicit ops stay strict ----------------------------------------------------------------------------------------------------------------
def _layout_of(consumer, shape, dtype, seed):
    """A device tensor in the layout the consumer hands ``out`` (torch.autograd.grad of the consumer on a device leaf)."""
    x = torch.zeros(shape, dtype=dtype, device=DEV, requires_grad=True)
    (d,) = torch.autograd.grad(consumer.y(x), x, AL.upstream(consumer, shape, dtype, seed).to(DEV))
    assert (tuple(d.stride()), d.storage_offset()) == consumer.strides(*shape)
    return d


@pytest.mark.parametrize("kind", ["fixed", "varlen"])
def test_explicit_backward_ops_still_refuse(tfa, kind):
    """ops.flash_attn_bwd / flash_attn_varlen_bwd do not copy: the row-stride-0, the misaligned and the head-padded gradient are refused with the stride /
    alignment status, before any launch."""
    from tiny_flash_attention_amd import _lib, ops

    t = problem(PLAIN if kind == "fixed" else VARLEN_PLAIN)
    c, sc = t["case"], t["sc"]
    if kind == "fixed":
        q, k, v = (t[n].transpose(1, 2).contiguous().to(DEV) for n in ("q", "k", "v"))
        out, lse = ops.flash_attn_fwd(q, k, v, c["causal"], sc, layout="bnhd")
        bwd = lambda do: ops.flash_attn_bwd(q, k, v, out, lse, do, c["causal"], sc, layout="bnhd")          # noqa: E731
    else:
        q, k, v = (t[n].to(DEV) for n in ("q", "k", "v"))
        cu = (t["cu_q"].to(DEV), t["cu_k"].to(DEV), max(c["lq"]), max(c["lk"]))
        out, lse = ops.flash_attn_varlen_fwd(q, k, v, *cu, c["causal"], sc)
        bwd = lambda do: ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, *cu, c["causal"], sc)             # noqa: E731
    shape = tuple(out.shape)
    for cid in AL.RAISED:
        do = _layout_of(AL.catalogue(shape)[cid], shape, out.dtype, 750)
        with pytest.raises(_lib.TfaError) as e:
            bwd(do)
        assert e.value.status == TFA_ERR_STRIDE, cid          # (strides are checked before bases)
    flat = torch.zeros(out.numel() + 8, dtype=out.dtype, device=DEV)
    with pytest.raises(_lib.TfaError) as e:
        bwd(flat[4:4 + out.numel()].view(shape))              # dense strides, a base 8 bytes into an allocation
    assert e.value.status == TFA_ERR_ALIGN
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g.float()).all()) for g in bwd(torch.zeros_like(out)))                  # the same call, a legal gradient: runs
