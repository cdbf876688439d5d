"""The tensor layouts autograd really hands the three autograd functions (flash_attn_func, flash_attn_varlen_func, apply_rotary_emb), as catalogues shared by
tests/test_autograd_layouts_cpu.py (which proves on the CPU that torch produces the strides each entry claims) and tests/test_autograd_layouts_gpu.py (tests only).

CONSUMERS / PACKED_CONSUMERS: what a model does with ``out`` (B, N, H, D) / packed (total, H, D).  Every consumer is a linear map y(out) that only selects,
repeats or sums elements, so the gradient it hands back for a seeded upstream g of y's shape is a VIEW of g: dense_dout gives its dense values exactly (no
arithmetic, nothing to round), and they feed the fp64 reference and the contiguous control run.  ``strides(*shape)`` is (strides, storage offset) of that view.
INPUT_VIEWS / PACKED_INPUT_VIEWS: how a model makes q, k, v — views of shared projection leaves.
"""
import collections

import torch

import form_ref as F

Consumer = collections.namedtuple("Consumer", "id y strides")


def _cat_flat_front4(o):
    """[4 other columns | every head of a row]: the gradient of ``out`` starts 4 elements into the upstream buffer and its rows are H * D + 4 apart."""
    return torch.cat([o.new_zeros(o.shape[:-2] + (4,)), o.flatten(-2)], dim=-1)


def _cat_head_pad4(o):
    """4 more columns behind every head: heads D + 4 apart."""
    return torch.cat([o, o.new_zeros(o.shape[:-1] + (4,))], dim=-1)


CONSUMERS = [
    Consumer("sum_rows", lambda o: o.sum(1), lambda B, N, H, D: ((H * D, 0, D, 1), 0)),
    Consumer("sum_batch", lambda o: o.sum(0), lambda B, N, H, D: ((0, H * D, D, 1), 0)),
    Consumer("sum_heads", lambda o: o.sum(2), lambda B, N, H, D: ((N * D, D, 0, 1), 0)),
    Consumer("sum_all", lambda o: o.sum(), lambda B, N, H, D: ((0, 0, 0, 0), 0)),
    Consumer("cat_flat_front4", _cat_flat_front4, lambda B, N, H, D: ((N * (H * D + 4), H * D + 4, D, 1), 4)),
    Consumer("cat_head_pad4", _cat_head_pad4, lambda B, N, H, D: ((N * H * (D + 4), H * (D + 4), D + 4, 1), 0)),
    Consumer("transposed", lambda o: o.transpose(1, 2), lambda B, N, H, D: ((H * N * D, D, N * D, 1), 0)),
    Consumer("d_first", lambda o: o.permute(0, 3, 1, 2), lambda B, N, H, D: ((D * N * H, H, 1, N * H), 0)),
]
PACKED_CONSUMERS = [
    Consumer("sum_rows", lambda o: o.sum(0), lambda T, H, D: ((0, D, 1), 0)),
    Consumer("sum_heads", lambda o: o.sum(1), lambda T, H, D: ((D, 0, 1), 0)),
    Consumer("sum_all", lambda o: o.sum(), lambda T, H, D: ((0, 0, 0), 0)),
    Consumer("cat_flat_front4", _cat_flat_front4, lambda T, H, D: ((H * D + 4, D, 1), 4)),
    Consumer("cat_head_pad4", _cat_head_pad4, lambda T, H, D: ((H * (D + 4), D + 4, 1), 0)),
    Consumer("transposed", lambda o: o.transpose(0, 1), lambda T, H, D: ((D, T * D, 1), 0)),
    Consumer("d_first", lambda o: o.permute(2, 0, 1), lambda T, H, D: ((H, 1, T * H), 0)),
]
BY_ID = {c.id: c for c in CONSUMERS}
PACKED_BY_ID = {c.id: c for c in PACKED_CONSUMERS}
RAISED = ("sum_rows", "cat_flat_front4", "cat_head_pad4")     # refused by tfa_bwd / tfa_bwd_varlen: the autograd functions used to pass them on and raise


def catalogue(shape):
    return BY_ID if len(shape) == 4 else PACKED_BY_ID


def abi_takes(strides, offset, D, esize=2):
    """The C ABI's rule for a backward operand (csrc/tfa_bwd_api.hip: check_strides, check_bwd) on a gradient shaped like ``out``: unit stride along D, every other
    stride >= 0 and a multiple of 16 bytes, the row stride (dim 1 of (B, N, H, D), dim 0 of (total, H, D)) >= D, a 16-byte base (offset: elements into an
    allocation, which torch aligns to more than that)."""
    row = strides[1] if len(strides) == 4 else strides[0]
    return strides[-1] == 1 and all(s >= 0 and (s * esize) % 16 == 0 for s in strides[:-1]) and row >= D and (offset * esize) % 16 == 0


def upstream(consumer, shape, dtype, seed):
    """The seeded upstream gradient of the consumer's y, on the CPU."""
    return F.rnd(tuple(consumer.y(torch.zeros(shape, dtype=dtype)).shape), dtype, seed)


def dense_dout(consumer, shape, g):
    """The gradient the consumer hands ``out`` for the upstream g (a CPU tensor), dense: torch.autograd.grad of the consumer itself on the CPU.  Exact in g's
    dtype — every consumer only selects, repeats or drops elements of g."""
    o = torch.zeros(shape, dtype=g.dtype, requires_grad=True)
    (d,) = torch.autograd.grad(consumer.y(o), o, g)
    return d.contiguous()


# ---- inputs as views of shared leaves ---------------------------------------------------------------------------------------------------------
# leaves(B, Nq, Nk, H, Hk, D) -> the leaf shapes; views(leaves, B, Nq, Nk, H, Hk, D) -> (q, k, v); fused: q and k share rows (Nq == Nk);
# hk(H, Hk): the K/V heads the call sees.  Packed: the same with (Tq, Tk, H, Hk, D).
View = collections.namedtuple("View", "id leaves views fused hk")


def _offset16_sizes(B, Nq, Nk, H, Hk, D):
    nq, nk = B * Nq * H * D, B * Nk * Hk * D
    return nq, nk, (16, 16 + nq + 8, 16 + nq + 8 + nk + 24)          # element offsets of q, k, v: non-zero multiples of 8


def _offset16_leaves(B, Nq, Nk, H, Hk, D):
    nq, nk, off = _offset16_sizes(B, Nq, Nk, H, Hk, D)
    return [(off[2] + nk + 8,)]


def _offset16_views(ls, B, Nq, Nk, H, Hk, D):
    nq, nk, off = _offset16_sizes(B, Nq, Nk, H, Hk, D)
    buf = ls[0]
    return (buf[off[0]:off[0] + nq].view(B, Nq, H, D), buf[off[1]:off[1] + nk].view(B, Nk, Hk, D), buf[off[2]:off[2] + nk].view(B, Nk, Hk, D))


INPUT_VIEWS = [
    View("qkv3", lambda B, Nq, Nk, H, Hk, D: [(B, Nq, 3, H, D)], lambda ls, *_: ls[0].unbind(2), True, lambda H, Hk: H),
    View("qkv_gqa", lambda B, Nq, Nk, H, Hk, D: [(B, Nq, H + 2 * Hk, D)],
         lambda ls, B, Nq, Nk, H, Hk, D: (ls[0][:, :, :H], ls[0][:, :, H:H + Hk], ls[0][:, :, H + Hk:]), True, lambda H, Hk: Hk),
    View("kv2", lambda B, Nq, Nk, H, Hk, D: [(B, Nq, H, D), (B, Nk, 2, Hk, D)], lambda ls, *_: (ls[0],) + tuple(ls[1].unbind(2)), False, lambda H, Hk: Hk),
    View("k_heads_expanded", lambda B, Nq, Nk, H, Hk, D: [(B, Nq, H, D), (B, Nk, 1, D), (B, Nk, H, D)],
         lambda ls, B, Nq, Nk, H, Hk, D: (ls[0], ls[1].expand(B, Nk, H, D), ls[2]), False, lambda H, Hk: H),
    View("kv_batch_expanded", lambda B, Nq, Nk, H, Hk, D: [(B, Nq, H, D), (1, Nk, Hk, D), (1, Nk, Hk, D)],
         lambda ls, B, Nq, Nk, H, Hk, D: (ls[0], ls[1].expand(B, Nk, Hk, D), ls[2].expand(B, Nk, Hk, D)), False, lambda H, Hk: Hk),
    View("offset16", _offset16_leaves, _offset16_views, False, lambda H, Hk: Hk),
]
PACKED_INPUT_VIEWS = [
    View("qkv3", lambda Tq, Tk, H, Hk, D: [(Tq, 3, H, D)], lambda ls, *_: ls[0].unbind(1), True, lambda H, Hk: H),
    View("qkv_gqa", lambda Tq, Tk, H, Hk, D: [(Tq, H + 2 * Hk, D)],
         lambda ls, Tq, Tk, H, Hk, D: (ls[0][:, :H], ls[0][:, H:H + Hk], ls[0][:, H + Hk:]), True, lambda H, Hk: Hk),
]
VIEW_BY_ID = {v.id: v for v in INPUT_VIEWS}
PACKED_VIEW_BY_ID = {v.id: v for v in PACKED_INPUT_VIEWS}


def build_view(view, dims, dtype, seed, device="cpu", std=0.5):
    """(leaves, (q, k, v) views of them, contiguous clones of the views as leaves of their own): seeded values, the leaves and the clones require grad."""
    leaves = [F.rnd(s, dtype, seed + i, std).to(device).requires_grad_(True) for i, s in enumerate(view.leaves(*dims))]
    qkv = view.views(leaves, *dims)
    clones = tuple(t.detach().clone(memory_format=torch.contiguous_format).requires_grad_(True) for t in qkv)
    return leaves, qkv, clones


def assemble(view, dims, leaves, grads):
    """The leaves' gradients given dq, dk, dv of the views, made with the torch ops autograd itself runs for the views (stack, slice, the sum of an expand):
    torch.autograd.grad through the same views of zero leaves."""
    zeros = [torch.zeros_like(l).requires_grad_(True) for l in leaves]
    return torch.autograd.grad(view.views(zeros, *dims), zeros, grads)
