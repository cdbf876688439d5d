"""The K/V-cache family on pools beyond 4 GiB: every case of kvcache_ref, kvcache_window_ref and kvcache_tree_ref, fwd_ref's paged cases, 16 seeded draws of each,
far_pool.EXTRA and the plain-launch appends run the public call with their caches placed far apart in one arena of 8 GiB + 64 MiB (tests/far_pool.py: the
engine's interleaved (num_pages, 2, page, Hk, D) pool with page indices at and around 2^31, 2^32 and 2^33 bytes; contiguous caches 2 to 8 GiB apart), so that the
offsets the kernels form — page * page_stride, b * batch_stride, in elements and in bytes — pass 32 bits.  tests/test_far_pool_cpu.py proves the placement: a
truncated offset of any placed slot lands in 0xFF bytes — NaN in every cache type — never in another slot.

Per case, through the call paths of tests/test_kvcache_fwd_bounds_gpu.py, test_kvcache_window_gpu.py, test_kvcache_tree_gpu.py and test_fwd_bounds_gpu.py (place=):
    the family's own per-element bounds against fp64 (out, lse, exact +inf and 0 on rows without keys, no NaN) on the far placement;
    out and lse bit-identical to the same case run from its small pool in the same test (the host plans both alike: test_far_pool_cpu.py; only addresses differ);
    the placed slots afterwards hold, byte for byte, what the call is defined to leave in them (an append: k_final / v_final, dropped rows stay dropped; no
    append: what they held);
    every other byte of the arena is still 0xFF (one read of the arena per test).
"""
import functools

import pytest
import torch

import far_pool as FP
import test_append_varlen_gpu as GA
import test_fwd_bounds_gpu as GF
import test_kvcache_fwd_bounds_gpu as GK
import test_kvcache_tree_gpu as GT
import test_kvcache_window_gpu as GW

pytestmark = pytest.mark.gpu
MODS = FP.modules()
GPU = {"kvcache": GK, "window": GW, "tree": GT}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    try:
        a = FP.Arena(dev)
    except RuntimeError as e:
        pytest.fail(str(e))                                # no skip: a test that never runs proves nothing
    yield a
    a.mem = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib():
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    yield _lib
    _lib.set_variant(-1)


@functools.lru_cache(maxsize=None)
def tensors(name, cid):
    """The case's tensors and its fp64 reference (the lists' cases: the ones the family's own GPU module computed, shared), and the placement."""
    if cid in FP.EXTRA_BY_ID:
        mod = MODS[name][0]
        t = mod.build(FP.EXTRA_BY_ID[cid])
        ref = mod.reference(t)
    else:
        t, ref = GPU[name].reference(cid)
    return t, ref, FP.place(t)


def after_the_call(arena, pl, what):
    """The placed slots against what the call is defined to leave in them, and the rest of the arena against 0xFF (the slots were taken out and reset by then)."""
    k_after, v_after = what
    assert arena.clean(), "a byte of the arena outside the placed slots changed"
    assert FP.same_bits(k_after, pl.L["kf"]), "the placed K slots do not hold what the call is defined to leave in them"
    assert FP.same_bits(v_after, pl.L["vf"]), "the placed V slots do not hold what the call is defined to leave in them"


def test_the_scrub_sees_a_single_changed_byte(arena):
    """Arena.clean — min and max of the arena as int64 — misses no byte, at either end or behind 2^31, 2^32 and 2^33."""
    assert arena.clean()
    for at in (0, 2 ** 31 + 3, 2 ** 32 + 5, 2 ** 33 + 7, FP.ARENA_BYTES - 1):
        for byte in (0xFE, 0x7F, 0x00):
            arena.mem[at] = byte
            assert not arena.clean(), (at, byte)
            arena.mem[at] = 0xFF
    assert arena.clean()


def run_far(name, cid, dev, arena):
    G = GPU[name]
    t, ref, pl = tensors(name, cid)
    small = G.call(t, dev)
    try:
        got = G.call(t, dev, place=arena.put(pl))
    finally:
        left = arena.take(pl)
    after_the_call(arena, pl, left)
    G.check(cid + " (far)", t, ref, got)
    assert GW.identical(got, small), f"{cid}: the far placement changes bits of out or lse"
    if t["case"]["append"] is not None:
        assert not FP.same_bits(pl.L["kf"], pl.L["kc"])


@pytest.mark.parametrize("cid", MODS["kvcache"][1])
def test_kvcache_forward(dev, arena, cid):
    run_far("kvcache", cid, dev, arena)


@pytest.mark.parametrize("cid", MODS["window"][1])
def test_windowed(dev, arena, cid):
    run_far("window", cid, dev, arena)


@pytest.mark.parametrize("cid", MODS["tree"][1])
def test_tree(dev, arena, cid):
    run_far("tree", cid, dev, arena)


@pytest.mark.parametrize("cid", MODS["prefill"][1])
def test_paged_prefill(dev, arena, lib, cid):
    t, _, _ = GF.reference(cid)
    pl = FP.place(t)
    small = GF.run_case(cid, dev, lib)
    try:
        far = GF.run_case(cid, dev, lib, place=lambda _t: arena.put(pl))
    finally:
        left = arena.take(pl)
    after_the_call(arena, pl, left)
    o16, o32, lses = far
    assert torch.equal(o16.view(torch.int16), small[0].view(torch.int16)) and torch.equal(o32, small[1]), f"{cid}: the far placement changes bits of out"
    n = int(t["cu_q"][-1])                                 # (the rows behind every sequence: out holds the sentinel, the LSE the call allocated is not written)
    assert all(torch.equal(a[:, :n], b[:, :n]) for a, b in zip(lses, small[2])), f"{cid}: the far placement changes bits of the LSE"


@pytest.mark.parametrize("page", [64, 0], ids=["paged", "contiguous"])
@pytest.mark.parametrize("kind", FP.APPEND_VARLEN)
def test_plain_launch_append(dev, arena, kind, page):
    """kvcache_append_varlen without q= and without fp8 — launch_kvcache_append_varlen — plain, with GPT-NeoX tables and with interleaved ones, over
    tests/test_append_varlen_gpu.py's geometry at a capacity of 192: the last sequence's rows at positions 192 .. 199 are dropped."""
    import tiny_flash_attention_amd as tfa

    assert (FP.NEW, FP.CACHED, FP.APPEND_HK) == (GA.NEW, GA.CACHED, GA.HK)
    t = FP.append_varlen_case(kind, page=page)
    pl = FP.place(t)
    d = lambda x: x.to(dev)      # noqa: E731
    kw = {} if kind == "plain" else dict(rotary_cos=d(t["cos"]), rotary_sin=d(t["sin"]), rotary_interleaved=kind == "interleaved")
    ks, vs = d(t["k_cache"]), d(t["v_cache"])
    tfa.kvcache_append_varlen(d(t["k_new"]), d(t["v_new"]), ks, vs, d(t["cu"]), d(t["before"]), None if t["bt"] is None else d(t["bt"]), **kw)
    torch.cuda.synchronize()
    assert FP.same_bits(ks.cpu(), t["k_final"]) and FP.same_bits(vs.cpu(), t["v_final"]), "the small pool is not what the append is defined to store"
    assert not FP.same_bits(t["k_final"], t["k_cache"]) and sum(min(a + n, 192) - a for a, n in zip(FP.CACHED, FP.NEW)) == sum(FP.NEW) - 8
    try:
        kc, vc, bt = arena.put(pl)
        tfa.kvcache_append_varlen(d(t["k_new"]), d(t["v_new"]), kc, vc, d(t["cu"]), d(t["before"]), bt, **kw)
        torch.cuda.synchronize()
    finally:
        left = arena.take(pl)
    after_the_call(arena, pl, left)
