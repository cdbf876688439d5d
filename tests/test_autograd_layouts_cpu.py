"""tests/autograd_layouts.py's catalogues are true of this torch (no GPU): each consumer hands an autograd.Function the strides and storage offset its entry
claims, dense_dout is that gradient made contiguous, and each input view has the strides the GPU tests mean to exercise.  A torch that starts materialising
these gradients would otherwise turn tests/test_autograd_layouts_gpu.py into repeats of the dense case without anyone noticing."""
import pytest
import torch

import autograd_layouts as AL

B, N, H, HK, D = 2, 5, 4, 2, 16
TOTAL = 11
SHAPES = {4: (B, N, H, D), 3: (TOTAL, H, D)}


class _Probe(torch.autograd.Function):
    """The identity, recording what autograd hands its backward."""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, dout):
        _Probe.seen = dout
        return dout


def _handed(consumer, shape, dtype, seed):
    g = AL.upstream(consumer, shape, dtype, seed)
    x = torch.zeros(shape, dtype=dtype, requires_grad=True)
    consumer.y(_Probe.apply(x)).backward(g)
    return g, _Probe.seen


CASES = [(4, c.id) for c in AL.CONSUMERS] + [(3, c.id) for c in AL.PACKED_CONSUMERS]


@pytest.mark.parametrize("rank,cid", CASES, ids=[f"{'bnhd' if r == 4 else 'packed'}-{c}" for r, c in CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_consumer_hands_the_layout_its_entry_claims(rank, cid, dtype):
    shape = SHAPES[rank]
    consumer = AL.catalogue(shape)[cid]
    g, dout = _handed(consumer, shape, dtype, seed=7)
    strides, offset = consumer.strides(*shape)
    assert tuple(dout.shape) == shape and dout.dtype == dtype
    assert (tuple(dout.stride()), dout.storage_offset()) == (strides, offset)
    dense = AL.dense_dout(consumer, shape, g)
    assert dense.is_contiguous() and dense.storage_offset() == 0
    assert torch.equal(dense.view(torch.int16), dout.contiguous().view(torch.int16))


def test_the_catalogue_spans_what_the_c_abi_takes_and_what_it_refuses():
    """By the ABI's rule the three consumers that used to raise are refused (and so is d_first, which always was copied); the transposed and the zero batch /
    head stride gradients are taken as they are."""
    for shape, cat in ((SHAPES[4], AL.BY_ID), (SHAPES[3], AL.PACKED_BY_ID)):
        takes = {cid: AL.abi_takes(*c.strides(*shape), D) for cid, c in cat.items()}
        assert not any(takes[c] for c in AL.RAISED + ("d_first", "sum_all")), takes
        assert all(takes[c] for c in cat if c not in AL.RAISED + ("d_first", "sum_all")), takes
    assert AL.BY_ID["cat_flat_front4"].strides(*SHAPES[4])[0][1] % 8 != 0 and AL.BY_ID["cat_flat_front4"].strides(*SHAPES[4])[1] % 8 != 0


def test_input_views_have_the_strides_they_are_named_for():
    dims = (B, N, N, H, HK, D)
    for view in AL.INPUT_VIEWS:
        leaves, (q, k, v), clones = AL.build_view(view, dims, torch.bfloat16, seed=3)
        hk = view.hk(H, HK)
        assert tuple(q.shape) == (B, N, H, D) and tuple(k.shape) == tuple(v.shape) == (B, N, hk, D), view.id
        for t, c in zip((q, k, v), clones):
            assert t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.storage_offset() % 8 == 0, view.id      # what the kernels take uncopied
            assert c.is_contiguous() and c.is_leaf and torch.equal(c.view(torch.int16), t.contiguous().view(torch.int16))
        assert all(l.is_leaf and l.requires_grad for l in leaves)
    _, (q, k, v), _ = AL.build_view(AL.VIEW_BY_ID["qkv3"], dims, torch.bfloat16, 3)
    assert q.stride() == (N * 3 * H * D, 3 * H * D, D, 1) and (k.storage_offset(), v.storage_offset()) == (H * D, 2 * H * D)
    _, (q, k, v), _ = AL.build_view(AL.VIEW_BY_ID["qkv_gqa"], dims, torch.bfloat16, 3)
    assert q.stride(1) == k.stride(1) == (H + 2 * HK) * D and (k.storage_offset(), v.storage_offset()) == (H * D, (H + HK) * D)
    _, (q, k, v), _ = AL.build_view(AL.VIEW_BY_ID["kv2"], dims, torch.bfloat16, 3)
    assert q.is_contiguous() and k.stride() == (N * 2 * HK * D, 2 * HK * D, D, 1) and v.storage_offset() == HK * D
    _, (q, k, v), _ = AL.build_view(AL.VIEW_BY_ID["k_heads_expanded"], dims, torch.bfloat16, 3)
    assert k.stride() == (N * D, D, 0, 1) and v.is_contiguous()
    _, (q, k, v), _ = AL.build_view(AL.VIEW_BY_ID["kv_batch_expanded"], dims, torch.bfloat16, 3)
    assert k.stride(0) == 0 and v.stride(0) == 0
    _, qkv, _ = AL.build_view(AL.VIEW_BY_ID["offset16"], dims, torch.bfloat16, 3)
    assert all(t.is_contiguous() and t.storage_offset() > 0 and t.storage_offset() % 8 == 0 for t in qkv)
    pdims = (TOTAL, TOTAL, H, HK, D)
    _, (q, k, v), _ = AL.build_view(AL.PACKED_VIEW_BY_ID["qkv3"], pdims, torch.bfloat16, 3)
    assert q.stride() == (3 * H * D, D, 1) and k.storage_offset() == H * D
    _, (q, k, v), _ = AL.build_view(AL.PACKED_VIEW_BY_ID["qkv_gqa"], pdims, torch.bfloat16, 3)
    assert tuple(k.shape) == (TOTAL, HK, D) and q.stride(0) == (H + 2 * HK) * D and v.storage_offset() == (H + HK) * D


def test_assemble_is_what_autograd_accumulates_into_the_leaves():
    """assemble(view, ...) of given dq, dk, dv equals the leaves' .grad after backward through the views, in bits — an expanded K sums its heads in 16 bit."""
    dims = (B, N, N, H, HK, D)
    for view in AL.INPUT_VIEWS:
        leaves, qkv, _ = AL.build_view(view, dims, torch.bfloat16, seed=5)
        grads = tuple(AL.F.rnd(tuple(t.shape), torch.bfloat16, 40 + i) for i, t in enumerate(qkv))
        torch.autograd.backward(qkv, grads)
        for l, a in zip(leaves, AL.assemble(view, dims, leaves, grads)):
            assert torch.equal(l.grad.view(torch.int16), a.view(torch.int16)), view.id
